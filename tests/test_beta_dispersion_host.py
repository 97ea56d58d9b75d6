"""The host side of the between-set dispersion reduction (no GPU): st_beta_dispersion_matrix(device = -1), the restatement of
the kernels' order rule, against the float64 brute force of tests/beta_dispersion_reference.py; its invariances and
degenerate cases; the plan under the sanitizers; argument checks of the library and the facade; the columns of
compare.SetBetaDispersion.

Bounds.  A direction adds k_r k_c float32 values (cross_sum) or k_r of them (nearest_sum), each exact in float64, in some
order: a sum of n doubles errs by at most n 2^-53 relative for non-negative terms.  The tests allow twice that --
k_r k_c 2^-52 and k_r 2^-52, relative -- against math.fsum, whose result is the correctly rounded sum."""
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import beta_dispersion_reference as ref
from conftest import ROOT, golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare, build as st_build


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()
    return _capi.load()


def _matrix(n, seed):
    """Seeded random float32 distances, as a tree's would be: positive, a few orders of magnitude, not symmetric."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, n)) * 10.0 ** rng.integers(-2, 2, (n, n))).astype(np.float32)


def _sets(n, sizes, seed):
    """One random set per size that fits, then the first half of the largest (nested in it) and the largest again."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in sizes if k <= n]
    big = max(sets, key=len)
    return sets + [big[: max(1, len(big) // 2)], big.copy()]


def _check_against_reference(D, sets, out, seed, stream, exclude, begin=0):
    """Every record of ``out`` (pairs from ``begin``) against the brute force, within the bounds of the module docstring."""
    n = len(D)
    worst = [0.0, 0.0]
    for p in range(out.shape[2]):
        sigma = compare.hommola_permutation(seed, stream, p, 0, n)
        for k, (i, j) in enumerate(ref.pairs(len(sets), begin, out.shape[0])):
            for d, (r, c) in enumerate(((i, j), (j, i))):
                cross, near, _ = ref.direction(D, sigma, sets[r], sets[c], exclude)
                got = out[k, d, p]
                kr, kc = len(sets[r]), len(sets[c])
                e_cross, e_near = abs(got["pair_sum"] - cross), abs(got["nearest_sum"] - near)
                assert e_cross <= kr * kc * 2.0 ** -52 * cross, (i, j, d, p, got, cross)      # (a sum of 0 -- nothing included, or a
                assert e_near <= kr * 2.0 ** -52 * near, (i, j, d, p, got, near)              # shared member at distance 0 -- is exact)
                worst = [max(worst[0], e_cross / (kr * kc * cross) if cross else 0.0), max(worst[1], e_near / (kr * near) if near else 0.0)]
    print("worst relative error in units of the bound: cross %.3g, nearest %.3g" % (worst[0] * 2.0 ** 52, worst[1] * 2.0 ** 52))


def test_worked_example():
    """D[a][b] = |a - b| on 5 positions, A = {0, 1, 4}, B = {1, 2}: the table of the header."""
    D = np.abs(np.arange(5)[:, None] - np.arange(5)[None, :]).astype(np.float32)
    A, B = [0, 1, 4], [1, 2]
    want = {False: ((9.0, 3.0), (9.0, 1.0), 1.5, 0.8), True: ((9.0, 4.0), (9.0, 2.0), 1.8, 1.2)}
    for exclude, (ab, ba, mpd, mntd) in want.items():
        rec = _capi.beta_dispersion_matrix(D, [B, A], exclude_shared=exclude)      # pair 0 is (i, j) = (A, B): A -> B, then B -> A
        assert rec.shape == (1, 2, 1)
        assert (rec[0, 0, 0]["pair_sum"], rec[0, 0, 0]["nearest_sum"]) == ab and (rec[0, 1, 0]["pair_sum"], rec[0, 1, 0]["nearest_sum"]) == ba
        out = compare.SetBetaDispersion(2, 0, 1, 0, 1, 5, exclude)
        out.fill(0, [3], [2], [1], rec)
        assert out.beta_mpd[0] == mpd and out.beta_mntd[0] == mntd and out.shared[0] == 1
        assert ref.beta(D, np.arange(5), A, B, exclude) == (mpd, mntd)
        assert ref.direction(D, np.arange(5), A, B, exclude)[:2] == ab


SIZES = (0, 1, 2, 3, 7, 8, 9, 32, 33, 64, 65, 257)


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("n", [3, 64, 65, 300])
def test_restatement_against_brute_force(n, exclude):
    D = _matrix(n, n)
    sets = _sets(n, SIZES, n + 1)
    perms, seed, stream = 2, 20250 + n, 4
    out = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=perms, seed=seed, stream=stream)
    assert out.shape == (len(sets) * (len(sets) - 1) // 2, 2, perms + 1)
    _check_against_reference(D, sets, out, seed, stream, exclude)


def _host_patristic(tree):
    """(leaf ids depth-first, the float32 patristic matrix over them) from the flat arrays, on the host: root depths in
    float64, the MRCA by marking ancestors."""
    parent, dist = np.asarray(tree._flat.parent), np.asarray(tree._flat.distance, dtype=np.float64)
    univ = tree._depth_first_leaves()
    lineage = []
    for leaf in univ.tolist():
        path, v = [], leaf
        while v != -1:
            path.append(v)
            v = int(parent[v])
        lineage.append(path[::-1])
    depth = {}
    for path in lineage:
        d = 0.0
        for v in path:
            d += dist[v] if parent[v] != -1 else 0.0
            depth[v] = d
    n = len(univ)
    D = np.zeros((n, n), dtype=np.float32)
    for a in range(n):
        for b in range(n):
            common = 0
            for x, y in zip(lineage[a], lineage[b]):
                if x != y:
                    break
                common = x
            D[a, b] = depth[lineage[a][-1]] + depth[lineage[b][-1]] - 2 * depth[common]
    return univ, D


@pytest.fixture(scope="module")
def fish_worm():
    """(D over the worm tree's leaves; position sets: the worms of six fish -- disjoint, a worm has one fish -- then the
    worms of each two neighbouring fish among them together, which overlap one another and hold the single ones)."""
    d = golden_path("fish_worm")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    worms = SuchTree(d + "/guest.tree")
    univ, D = _host_patristic(worms)
    where = {worms.leaf_nodes[int(v)]: k for k, v in enumerate(univ)}
    sets = [np.sort([where[w] for w in links.columns[links.loc[fish] > 0]]) for fish in links.index]
    sets = [s for s in sets if len(s)][:6]
    return D, sets + [np.union1d(a, b) for a, b in zip(sets, sets[1:])]


@pytest.mark.parametrize("exclude", [False, True])
def test_restatement_on_fish_worm(fish_worm, exclude):
    D, sets = fish_worm
    assert len(sets) == 11 and max(len(s) for s in sets) > 8
    assert any(len(np.intersect1d(sets[i], sets[j])) for i, j in ref.pairs(len(sets)))      # exclude_shared bites
    out = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=1, seed=7, stream=2)
    _check_against_reference(D, sets, out, 7, 2, exclude)


def test_invariances_as_bytes():
    n = 130
    D = _matrix(n, 5)
    sets = _sets(n, (2, 7, 40, 64, 65, 130, 1, 0), 6)
    sets = sets + [sets[2].copy(), sets[4].copy()]      # identical sets at other indices
    kw = dict(exclude_shared=True, seed=77, stream=3)
    full = _capi.beta_dispersion_matrix(D, sets, permutations=20, **kw)
    short = _capi.beta_dispersion_matrix(D, sets, permutations=5, **kw)
    assert np.ascontiguousarray(full[:, :, :6]).tobytes() == short.tobytes()                       # prefix in permutations
    total = len(short)
    for begin, count in ((0, 4), (4, 13), (17, total - 17), (total, 0), (2, 0)):                   # ranges cut mid-row
        part = _capi.beta_dispersion_matrix(D, sets, begin, count, permutations=5, **kw)
        assert part.tobytes() == np.ascontiguousarray(short[begin:begin + count]).tobytes(), (begin, count)
    for chunk in (1, 7):
        assert _capi.beta_dispersion_matrix(D, sets, permutations=5, chunk_tasks=chunk, **kw).tobytes() == short.tobytes()
    index = {pair: k for k, pair in enumerate(ref.pairs(len(sets)))}
    a, b = len(sets) - 2, len(sets) - 1                                                            # copies of sets 2 and 4
    assert short[index[(4, 2)]].tobytes() == short[index[(b, a)]].tobytes() == short[index[(b, 2)]].tobytes()      # identical pairs, identical bytes
    swapped = list(sets)
    swapped[2], swapped[4] = sets[4], sets[2]
    other = _capi.beta_dispersion_matrix(D, swapped, permutations=5, **kw)
    assert other[index[(4, 2)], 0].tobytes() == short[index[(4, 2)], 1].tobytes()                  # i and j swapped: the directions swap
    assert other[index[(4, 2)], 1].tobytes() == short[index[(4, 2)], 0].tobytes()
    alone = _capi.beta_dispersion_matrix(D, [sets[2], sets[4]], permutations=5, **kw)              # not on the other sets
    assert alone[0].tobytes() == short[index[(4, 2)]].tobytes()
    assert _capi.beta_dispersion_matrix(D, sets, permutations=5, seed=77, stream=4, exclude_shared=True)[:, :, 1:].tobytes() != short[:, :, 1:].tobytes()


def test_small_sets_and_the_structural_rule():
    D = np.round(_matrix(6, 8) * 64) / 64      # multiples of 1/64: every sum is exact
    sets = [[], [3], [3], [2], [1, 3, 5]]
    for exclude in (False, True):
        rec = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=3, seed=9)
        out = compare.SetBetaDispersion(5, 0, 10, 3, 9, 6, exclude)
        i, j = compare.SetUniFrac._rows(np.arange(10))
        k = np.array([len(s) for s in sets])
        bits = compare.set_bit_rows(np.concatenate([np.asarray(s, dtype=np.int64) for s in sets]), np.concatenate([[0], np.cumsum(k)]), 6)
        out.fill(0, k[i], k[j], compare.shared_counts(bits, i, j), rec)
        index = {pair: n for n, pair in enumerate(ref.pairs(5))}
        # an empty set: records of zeros in both directions, NaN statistics
        for other in (1, 4):
            assert rec[index[(other, 0)]].tobytes() == bytes(rec[0].nbytes)
            assert math.isnan(out.beta_mpd[index[(other, 0)]]) and math.isnan(out.beta_mntd[index[(other, 0)]])
        # {3} against {3}: one entry, D[3][3]; with exclude_shared no entry at all -- zeros, decided by the sets
        same = index[(2, 1)]
        if exclude:
            assert rec[same].tobytes() == bytes(rec[same].nbytes) and math.isnan(out.beta_mpd[same]) and math.isnan(out.beta_mntd[same])
        else:
            assert rec[same, 0, 0]["pair_sum"] == float(D[3, 3]) and out.beta_mntd[same] == float(D[3, 3])
        # {1, 3, 5} -> {3}: with exclude_shared element 3 has no entry and adds +0.0; {3} -> {1, 3, 5} walks the other two
        one = rec[index[(4, 1)], :, 0]
        if exclude:
            assert one[0]["pair_sum"] == float(D[1, 3]) + float(D[5, 3]) == one[0]["nearest_sum"]
            assert one[1]["pair_sum"] == float(D[3, 1]) + float(D[3, 5]) and one[1]["nearest_sum"] == float(min(D[3, 1], D[3, 5]))
            assert out.beta_mntd[index[(4, 1)]] == (one[0]["nearest_sum"] + one[1]["nearest_sum"]) / 3      # z = 1
            assert out.beta_mpd[index[(4, 1)]] == (one[0]["pair_sum"] + one[1]["pair_sum"]) / 4
        else:
            assert one[0]["pair_sum"] == float(D[1, 3]) + float(D[3, 3]) + float(D[5, 3])
            assert out.beta_mntd[index[(4, 1)]] == (one[0]["nearest_sum"] + one[1]["nearest_sum"]) / 4
        # {2} against {3}: single members that differ
        assert rec[index[(3, 1)], 0, 0]["pair_sum"] == float(D[2, 3]) and rec[index[(3, 1)], 1, 0]["nearest_sum"] == float(D[3, 2])
        for at, (a, b) in enumerate(ref.pairs(5)):      # every pair's statistics: exact, the sums being exact
            want, got = ref.beta(D, np.arange(6), sets[a], sets[b], exclude), (out.beta_mpd[at], out.beta_mntd[at])
            assert all((math.isnan(w) and math.isnan(g)) or w == g for w, g in zip(want, got)), (a, b, want, got)
    # the rule is structural: an included +inf minimum is kept as +inf, not taken for "no entry"
    E = np.full((3, 3), np.inf, dtype=np.float32)
    r = _capi.beta_dispersion_matrix(E, [[0], [1]])[0, :, 0]
    assert r["nearest_sum"].tolist() == [math.inf, math.inf] and r["pair_sum"].tolist() == [math.inf, math.inf]


def test_special_values_follow_the_comparison_rule():
    inf, nan = np.inf, np.nan
    D = np.array([[0, nan, 2.0, 5.0], [inf, 0, inf, inf], [-0.0, 0.0, 0, 1.0], [nan, nan, nan, 0]], dtype=np.float32)
    for a, b in (([0, 1], [1, 2, 3]), ([2], [0, 1]), ([3], [0, 1, 2]), ([0, 1, 2, 3], [0, 1, 2, 3])):
        for exclude in (False, True):
            got = _capi.beta_dispersion_matrix(D, [b, a], exclude_shared=exclude)[0, 0, 0]      # a -> b
            total_sum, total_near = 0.0, 0.0
            for i in a:
                m, total = np.float32(inf), 0.0
                for j in b:
                    if not (exclude and i == j):
                        v = D[i, j]
                        total += float(v)
                        m = v if v < m else m      # (a NaN is never taken; +inf stays unless something is smaller)
                total_sum += total
                total_near += float(m)
            assert (math.isnan(total_sum) and math.isnan(got["pair_sum"])) or got["pair_sum"] == total_sum, (a, b, exclude, got)
            assert got["nearest_sum"] == total_near, (a, b, exclude, got)
    # -0.0 then +0.0: the first of equal values stays, and -0.0 plus the absent lane's +0.0 is +0.0
    z = _capi.beta_dispersion_matrix(D, [[0, 1], [2]])[0, 0, 0]      # {2} -> {0, 1}: -0.0, 0.0
    assert z["nearest_sum"] == 0.0 and not math.copysign(1.0, z["nearest_sum"]) < 0 and z["pair_sum"] == 0.0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_setpair_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_setpair")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_setpair.cpp"), os.path.join(csrc, "setpair_plan.cpp"),
                           os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize setpair ok" in out.stdout


def _raw(D, n, pos, off, n_sets, begin, count, perms, stream, chunk, device=-1, out=True, n_pos=None):
    L = _capi.load()
    D = None if D is None else np.ascontiguousarray(D, dtype=np.float32)
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    rec = np.zeros((max(min(count, 16), 1), 2, min(max(perms, 0), 16) + 1), dtype=_capi.DISPERSION_RECORD)      # (room for every call that succeeds)
    p = _capi._ptr
    n_pos = (0 if pos is None else len(pos)) if n_pos is None else n_pos
    return L.st_beta_dispersion_matrix(device, p(D), n, p(pos), n_pos, p(off), n_sets, begin, count, 1, perms, 1, stream,
                                       chunk, p(rec) if out else None)


def test_library_argument_errors_in_the_stated_order():
    D = _matrix(5, 1)
    ok = ([0, 2, 4, 1, 3], [0, 3, 5, 5])      # three sets: three pairs
    assert _raw(D, 5, *ok, 3, 0, 3, 3, 0, 0) == _capi.ST_OK
    assert _raw(D, 5, *ok, 3, 3, 0, 3, 0, 0) == _capi.ST_OK      # an empty range at the end of the triangle
    big = 1 << 40
    # every case breaks its own check and every later one it can: the message is the first check's
    cases = [
        ("universe below 3", (D, 2, [0, 9], [0, 2], 1, -1, -1, -1, -1, -1), "universe"),
        ("universe above the limit", (D, _capi.HOMMOLA_MAX_UNIVERSE + 1, *ok, 3, -1, 0, -1, -1, -1), "universe"),
        ("negative permutations", (D, 5, [0, 9], [0, 2], 1, -1, -1, -1, -1, -1), "permutations < 0"),
        ("negative chunk_tasks", (D, 5, [0, 9], [0, 2], 1, -1, -1, 3, -1, -1), "chunk_tasks < 0"),
        ("negative stream", (D, 5, [0, 9], [0, 2], 1, -1, -1, 3, -1, 0), "stream < 0"),
        ("negative n_sets", (D, 5, *ok, -1, -1, 0, 3, 0, 0), "negative size"),
        ("NULL sets", (D, 5, ok[0], None, 3, -1, 0, 3, 0, 0), "NULL"),
        ("NULL positions", (D, 5, None, ok[1], 3, -1, 0, 3, 0, 0), "NULL"),
        ("offsets go back", (D, 5, ok[0], [0, 3, 2, 5], 3, -1, 0, 3, 0, 0), "offsets"),
        ("offsets past the positions", (D, 5, ok[0], [0, 3, 5, 6], 3, -1, 0, 3, 0, 0), "offsets"),
        ("position outside", (D, 5, [0, 2, 5, 1, 3], ok[1], 3, -1, 0, 3, 0, 0), "outside the universe"),
        ("unsorted set", (D, 5, [0, 4, 2, 1, 3], ok[1], 3, -1, 0, 3, 0, 0), "increasing"),
        ("duplicate", (D, 5, [0, 2, 2, 1, 3], ok[1], 3, 0, -1, 3, 0, 0), "increasing"),
        ("negative begin", (D, 5, *ok, 3, -1, 9, 3, 0, 0), "negative triangle range"),
        ("negative count", (D, 5, *ok, 3, 9, -1, 3, 0, 0), "negative triangle range"),
        ("begin past the triangle", (D, 5, *ok, 3, 4, 0, 3, 0, 0), "of a triangle of 3"),
        ("range past the triangle", (D, 5, *ok, 3, 2, 2, big, 0, 0), "of a triangle of 3"),
    ]
    for what, args, text in cases:
        assert _raw(*args, n_pos=5 if what == "NULL positions" else None) == _capi.ST_ERR_ARG, what
        assert text in _capi.last_error(), (what, _capi.last_error())
    # more than 2^31 pairs, then more than 2^40 records: 70000 empty sets make a triangle of 2.4e9 pairs
    many = np.zeros(70001, dtype=np.int64)
    assert _raw(D, 5, None, many, 70000, 0, (1 << 31) + 1, big, 0, 0) == _capi.ST_ERR_ARG and "2^31 pairs" in _capi.last_error()
    assert _raw(D, 5, None, many, 70000, 0, 1 << 20, 1 << 19, 0, 0) == _capi.ST_ERR_ARG and "2^40 records" in _capi.last_error()
    # behind the plan: the device, the matrix, the output
    for what, args in {"device below -1": (D, 5, *ok, 3, 0, 3, 3, 0, 0, -2), "NULL matrix": (None, 5, *ok, 3, 0, 3, 3, 0, 0),
                       "NULL out": (D, 5, *ok, 3, 0, 3, 3, 0, 0, -1, False)}.items():
        assert _raw(*args) == _capi.ST_ERR_ARG, what
        assert _capi.last_error(), what
    assert _raw(D, 5, *ok, 3, 1, 0, 3, 0, 0, -1, False) == _capi.ST_OK      # no pair: out may be NULL
    L = _capi.load()      # the tree entry refuses its own arguments before it looks at the tree
    pos, off, univ = np.array(ok[0], dtype=np.int32), np.array(ok[1], dtype=np.int64), np.arange(5, dtype=np.int64)
    rec = np.zeros((3, 2, 4), dtype=_capi.DISPERSION_RECORD)
    bad = _capi.ctypes.c_int64(0)
    p = _capi._ptr
    tail = (p(pos), 5, p(off), 3, 0, 3, 0, 3, 1, 0, 0, p(rec), _capi.ctypes.byref(bad))      # (the sets, the range, ..., out, bad_id)
    assert L.st_beta_dispersion_host(None, p(univ), 2, *tail) == _capi.ST_ERR_ARG and "universe" in _capi.last_error()
    assert L.st_beta_dispersion_host(None, None, 5, *tail) == _capi.ST_ERR_ARG and "univ is NULL" in _capi.last_error()
    assert L.st_beta_dispersion_host(None, p(univ), 5, *tail) == _capi.ST_ERR_ARG and "tree is NULL" in _capi.last_error()
    with pytest.raises(ValueError):
        _capi.beta_dispersion_matrix(D, [[0, 7], [1]])
    with pytest.raises(ValueError):
        _capi.beta_dispersion_matrix(D[:4], [[0, 1], [2]])
    with pytest.raises(ValueError):
        _capi.beta_dispersion_matrix(D, [[1, 0], [2]])      # the library's own check: not increasing
    with pytest.raises(ValueError):
        _capi.beta_dispersion_matrix(D, [[0, 1], [2]], begin=0, count=2)


@pytest.mark.parametrize("exclude", [False, True])
def test_result_columns_against_the_reference(exclude):
    n, perms, seed, stream = 40, 29, 5, 1
    D = _matrix(n, 12)
    sets = _sets(n, (1, 2, 5, 12, 40), 13) + [np.arange(n)]      # (the largest twice: a pair of whole universes)
    begin, count = 3, 17      # (pair 19 = (6, 4), both the whole universe, is inside)
    rec = _capi.beta_dispersion_matrix(D, sets, begin, count, exclude, perms, seed, stream)
    out = compare.SetBetaDispersion(len(sets), begin, count, perms, seed, n, exclude, keep_null=True)
    pos, off, _ = _capi._dispersion_sets(sets, n)
    i, j = compare.SetUniFrac._rows(begin + np.arange(count))
    k = np.diff(off)
    out.fill(0, k[i], k[j], compare.shared_counts(compare.set_bit_rows(pos, off, n), i, j), rec)
    assert len(out) == count and out.begin == begin and out.permutations == perms and out.seed == seed and out.n_universe == n
    sigmas = [compare.hommola_permutation(seed, stream, p, 0, n) for p in range(perms + 1)]
    whole_pairs = 0
    for at, (a, b) in enumerate(ref.pairs(len(sets), begin, count)):
        assert out.pair(at) == (a, b) and out.n_i[at] == len(sets[a]) and out.n_j[at] == len(sets[b])
        assert out.shared[at] == len(np.intersect1d(sets[a], sets[b]))
        draws = np.array([ref.beta(D, s, sets[a], sets[b], exclude) for s in sigmas])
        tol = 4 * len(sets[a]) * len(sets[b]) * 2.0 ** -52
        for col, name in enumerate(("beta_mpd", "beta_mntd")):
            got = getattr(out, name)[at]
            assert abs(got - draws[0, col]) <= tol * draws[0, col], (a, b, name)
            np.testing.assert_allclose(getattr(out, "null_" + name)[at], draws[1:, col], rtol=tol)
            if len(sets[a]) == n and len(sets[b]) == n:      # both the whole universe: the null is the observation
                whole_pairs += col == 0
                assert getattr(out, name + "_null_mean")[at] == got and getattr(out, name + "_null_sd")[at] == 0.0
                assert math.isnan(getattr(out, name + "_ses")[at]) and getattr(out, name + "_p_le")[at] == 1.0 == getattr(out, name + "_p_ge")[at]
                continue
            want = ref.null_columns(got, getattr(out, "null_" + name)[at])      # (from the kept draws: counts compare equal values)
            for suffix, v in want.items():
                g = getattr(out, name + suffix)[at]
                assert (math.isnan(v) and math.isnan(g)) or abs(g - v) <= 1e-9 * max(1.0, abs(v)), (a, b, name + suffix, g, v)
    assert whole_pairs == 1 and (out.n_nan == 0).all()
    assert list(out.to_dataframe().columns) == ["i", "j"] + list(compare.SetBetaDispersion.COLUMNS) and out.row(3)["i"] == out.pair(3)[0]
    with pytest.raises(ValueError):
        out.matrix("beta_mntd")      # not the whole triangle
    with pytest.raises(IndexError):
        out.pair(count)
    rec = _capi.beta_dispersion_matrix(D, sets[:4], permutations=3, seed=seed)
    full = compare.SetBetaDispersion(4, 0, 6, 3, seed, n)
    i, j = compare.SetUniFrac._rows(np.arange(6))
    full.fill(0, k[i], k[j], np.zeros(6, dtype=np.int64), rec)
    M = full.matrix("beta_mpd")
    assert M.shape == (4, 4) and (M == M.T).all() and M[2, 1] == full.beta_mpd[2] and (np.diag(M) == 0).all()
    with pytest.raises(ValueError):
        full.matrix("n_i")


def _linked():
    from suchtree_amd import synth
    ta = SuchTree(synth.random_binary_tree(6, seed=1) + (["a%d" % i for i in range(6)],))
    tb = SuchTree(synth.random_binary_tree(9, seed=2) + (["b%d" % i for i in range(9)],))
    m = np.zeros((6, 9), dtype=int)
    m[0, :4] = m[1, 3:6] = m[2, 8] = 1
    links = pd.DataFrame(m, index=list(ta.leaves.keys()), columns=list(tb.leaves.keys()))
    return ta, tb, SuchLinkedTrees(ta, tb, links)


def test_facade_errors_raised_before_any_upload():
    from suchtree_amd.exceptions import NodeNotFoundError
    ta, tb, slt = _linked()
    for kw in ({"of": "C"}, {"pool": "all"}, {"permutations": -1}, {"permutations": 2.5}, {"permutations": True}, {"seed": -1}, {"seed": 1 << 64},
               {"min_partners": -1}, {"max_partners": 1.5}, {"begin": -1}, {"count": -1}, {"begin": 4}, {"begin": 2, "count": 2}, {"count": 1.5}):
        with pytest.raises(ValueError):
            slt.partner_beta_dispersion(**kw)
    names = list(tb.leaves.keys())
    two = [[names[0], names[1]], [names[2]]]
    for kw in ({"sets": [[names[0], names[0]], [names[1]]]},                  # a repeated member
               {"sets": two, "universe": names[1:5]},                         # a member outside the universe
               {"sets": two, "universe": names[:2]},                          # a universe below 3
               {"sets": [[tb.root_node, tb.leaves[names[0]]], [names[1]]]},   # an id that is no leaf
               {"sets": two, "stream": -1}, {"sets": two, "chunk_tasks": -1}, {"sets": two, "stream": 1 << 31},
               {"sets": two, "begin": 2}, {"sets": two, "count": 2}, {"sets": two, "begin": 1, "count": 1}):
        with pytest.raises(ValueError):
            tb.beta_dispersion(**kw)
    with pytest.raises(NodeNotFoundError):
        tb.beta_dispersion([["nobody"], [names[0]]])
    # no pair: nothing is launched, and neither tree goes to a device
    none = slt.partner_beta_dispersion(of="A", min_partners=4)      # one row
    assert len(none) == 0 and len(none.leaves) == 1 and none.names == ["a0"] and none.n_universe == 9 and none.n_sets == 1
    assert len(slt.partner_beta_dispersion(of="A", begin=3, permutations=3)) == 0
    assert len(tb.beta_dispersion([], permutations=3)) == 0 and len(tb.beta_dispersion([[names[0]]], permutations=3)) == 0
    assert len(tb.beta_dispersion(two, begin=1, permutations=3)) == 0
    assert ta._dev_tree is None and tb._dev_tree is None


def test_whole_triangle_above_2_31_pairs_is_refused():
    tb = _linked()[1]
    name = next(iter(tb.leaves))
    with pytest.raises(ValueError, match="more than 2\\^31"):
        tb.beta_dispersion([[name]] * 70000, permutations=0)
