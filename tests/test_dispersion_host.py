"""The host side of the partner-dispersion reduction (no GPU): st_dispersion_matrix(device = -1), the restatement of the
kernels' order rule, against a straightforward O(k^2) loop; its permutations, invariances and degenerate cases; the
taxa-labels null against independent draws; the plan under the sanitizers; argument checks of the library and facade.

Bounds.  A record adds k (k - 1) float32 values (pair_sum) or k of them (nearest_sum), each exact in float64, in some
order: every partial sum is rounded once, relative 2^-53, and for non-negative terms the total error is below
(number of adds) x 2^-53 x the sum.  The tests allow twice that -- k^2 2^-52 for MPD, k 2^-52 for MNTD, relative -- against
math.fsum, whose result is the correctly rounded sum."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dispersion_reference import plain as _plain      # (the O(k^2) math.fsum loop, shared with tests/fuzz_analyses.py)
from suchtree_amd import _capi, compare, build as st_build


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()
    return _capi.load()


def _matrix(n, seed):
    """Seeded random float32 distances, as a tree's would be: positive, a few orders of magnitude, not symmetric."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, n)) * 10.0 ** rng.integers(-2, 2, (n, n))).astype(np.float32)


def _sets(n, sizes, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, k, replace=False)) for k in sizes if k <= n]


SIZES = (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("n", [3, 64, 65, 300])
def test_restatement_against_plain_loop(n):
    D = _matrix(n, n)
    sets = _sets(n, SIZES, n + 1)
    perms, seed, stream = 3, 20240 + n, 4
    out = _capi.dispersion_matrix(D, sets, perms, seed, stream=stream)
    assert out.shape == (len(sets), perms + 1)
    for p in range(perms + 1):
        sigma = compare.hommola_permutation(seed, stream, p, 0, n)
        for r, s in enumerate(sets):
            k = len(s)
            want_pair, want_near = _plain(D, sigma[s])
            got = out[r, p]
            if k < 2:
                assert got["pair_sum"] == 0.0 and got["nearest_sum"] == 0.0
                continue
            mpd, want_mpd = got["pair_sum"] / (k * (k - 1)), want_pair / (k * (k - 1))
            mntd, want_mntd = got["nearest_sum"] / k, want_near / k
            print("n %d k %d p %d: mpd rel err %.3g (bound %.3g), mntd rel err %.3g (bound %.3g)"
                  % (n, k, p, abs(mpd - want_mpd) / want_mpd, k * k * 2.0 ** -52, abs(mntd - want_mntd) / want_mntd, k * 2.0 ** -52))
            assert abs(mpd - want_mpd) <= k * k * 2.0 ** -52 * want_mpd
            assert abs(mntd - want_mntd) <= k * 2.0 ** -52 * want_mntd


def test_special_values_follow_the_comparison_rule():
    inf, nan = np.inf, np.nan
    D = np.array([[0, nan, 2.0, 5.0], [inf, 0, inf, inf], [-0.0, 0.0, 0, 1.0], [nan, nan, nan, 0]], dtype=np.float32)
    for members in ([0, 1, 2], [0, 1, 2, 3], [2, 3], [1, 2]):
        got = _capi.dispersion_matrix(D, [members], 0, 1)[0, 0]
        k = len(members)
        rows = []
        for i in members:
            m, total = np.float32(inf), 0.0
            for j in members:
                if j != i:
                    v = D[i, j]
                    total += float(v)
                    m = v if v < m else m      # (a NaN is never taken; +inf stays unless something is smaller)
            rows.append((total, float(m)))
        want_pair, want_near = sum(t for t, _ in rows), sum(m for _, m in rows)
        assert (math.isnan(want_pair) and math.isnan(got["pair_sum"])) or got["pair_sum"] == want_pair, (members, got)
        assert got["nearest_sum"] == want_near, (members, got, k)
    # -0.0 then +0.0: the first of equal values stays, and the sum of the two minima is +0.0
    z = _capi.dispersion_matrix(np.array([[0, -0.0, 1], [0.0, 0, 1], [1, 1, 0]], dtype=np.float32), [[0, 1]], 0, 1)[0, 0]
    assert z["nearest_sum"] == 0.0 and not math.copysign(1.0, z["nearest_sum"]) < 0


@pytest.mark.parametrize("n", [3, 64, 65, 2049])
def test_sigma_is_the_hommola_permutation(n):
    """Position i of the universe moves to compare.hommola_permutation(seed, stream, p, 0, N)[i]: with D[a][b] = N a + b a pair
    set {i, j} returns the relabelled positions themselves."""
    seed, stream, perms = 31337 + n, 9, 4
    D = (np.arange(n, dtype=np.float32)[:, None] * n + np.arange(n, dtype=np.float32)[None, :])      # (exact: below 2^24)
    pairs = [(0, 1), (1, 2), (0, n - 1), (n // 2, n - 1)]
    out = _capi.dispersion_matrix(D, [list(s) for s in pairs], perms, seed, stream=stream)
    for p in range(perms + 1):
        sigma = compare.hommola_permutation(seed, stream, p, 0, n).astype(np.int64)
        if p == 0:
            assert (sigma == np.arange(n)).all()
        for r, (i, j) in enumerate(pairs):
            a, b = sigma[i], sigma[j]
            assert out[r, p]["pair_sum"] == float(n * a + b) + float(n * b + a)
    other = _capi.dispersion_matrix(D, [list(s) for s in pairs], perms, seed, stream=stream + 1)
    assert (other[:, 0] == out[:, 0]).all() and (other[:, 1:] != out[:, 1:]).any()      # the stream is part of the key


def test_prefix_identical_sets_and_chunks():
    n = 130
    D = _matrix(n, 5)
    sets = _sets(n, (2, 7, 40, 64, 65, 130, 1), 6)
    sets = sets + [sets[2], sets[4], sets[0]]      # identical sets at other indices
    full = _capi.dispersion_matrix(D, sets, 50, 77, stream=3)
    short = _capi.dispersion_matrix(D, sets, 5, 77, stream=3)
    assert full[:, :6].tobytes() == short.tobytes()
    assert full[2].tobytes() == full[7].tobytes() and full[4].tobytes() == full[8].tobytes() and full[0].tobytes() == full[9].tobytes()
    alone = _capi.dispersion_matrix(D, [sets[4]], 50, 77, stream=3)      # a record does not depend on the other sets
    assert alone[0].tobytes() == full[4].tobytes()
    for chunk in (1, 7):
        assert _capi.dispersion_matrix(D, sets, 5, 77, stream=3, chunk_tasks=chunk).tobytes() == short.tobytes()


def test_degenerate_sets():
    n = 12
    D = np.round(_matrix(n, 8) * 64) / 64      # multiples of 1/64: every sum is exact, whatever its order
    rec = _capi.dispersion_matrix(D.astype(np.float32), [list(range(n)), [3], [], [2, 9]], 20, 5)
    out = compare.SetDispersion(4, 20, 5, n, keep_null=True)
    out.fill(0, [n, 1, 0, 2], rec)
    # k = N: every shuffle gives the set itself
    assert (out.null_mpd[0] == out.mpd[0]).all() and out.mpd_null_sd[0] == 0.0 and math.isnan(out.mpd_ses[0]) and out.mpd_p[0] == 1.0
    assert out.mntd_null_sd[0] == 0.0 and math.isnan(out.mntd_ses[0]) and out.mntd_p[0] == 1.0
    # k < 2: a record of zeros, NaN statistics
    assert rec[1].tobytes() == bytes(rec[1].nbytes) and rec[2].tobytes() == bytes(rec[2].nbytes)
    assert math.isnan(out.mpd[1]) and math.isnan(out.mntd[2]) and math.isnan(out.mpd_p[1]) and out.n.tolist() == [n, 1, 0, 2]
    # k = 2: MPD = MNTD = the mean of the two directions
    assert out.mpd[3] == out.mntd[3] == (float(D[2, 9]) + float(D[9, 2])) / 2
    assert 0 < out.mpd_p[3] <= 1 and out.mpd_null_sd[3] > 0 and out.row(3)["n"] == 2
    assert list(out.to_dataframe().columns) == list(compare.SetDispersion.COLUMNS)


def _ks(a, b):
    """The two-sample Kolmogorov-Smirnov distance."""
    both = np.sort(np.concatenate([a, b]))
    return np.abs(np.searchsorted(np.sort(a), both, side="right") / len(a) - np.searchsorted(np.sort(b), both, side="right") / len(b)).max()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_null_against_independent_draws(seed):
    n, k, perms = 60, 7, 9999
    D = _matrix(n, 100 + seed)
    rec = _capi.dispersion_matrix(D, [np.sort(np.random.default_rng(50 + seed).choice(n, k, replace=False))], perms, seed)
    null_mpd = rec[0, 1:]["pair_sum"] / (k * (k - 1))
    rng = np.random.default_rng(seed)
    D64 = D.astype(np.float64)
    draws = np.empty(perms)
    for i in range(perms):
        s = rng.choice(n, k, replace=False)
        sub = D64[np.ix_(s, s)]
        draws[i] = (sub.sum() - np.trace(sub)) / (k * (k - 1))
    d = _ks(null_mpd, draws)
    bound = 1.95 * math.sqrt(2 / 9999)      # alpha = 0.001
    print("seed %d: KS distance %.4f, bound %.4f" % (seed, d, bound))
    assert d < bound


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dispersion_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_dispersion")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_dispersion.cpp"), os.path.join(csrc, "dispersion_plan.cpp"),
                           os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize dispersion ok" in out.stdout


def _raw(D, n, pos, off, n_sets, perms, stream, chunk, device=-1, out=True):
    L = _capi.load()
    D = None if D is None else np.ascontiguousarray(D, dtype=np.float32)
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    rec = np.zeros((max(n_sets, 1), max(perms, 0) + 1), dtype=_capi.DISPERSION_RECORD)
    p = _capi._ptr
    return L.st_dispersion_matrix(device, p(D), n, p(pos), 0 if pos is None else len(pos), p(off), n_sets, perms, 1, stream, chunk,
                                  p(rec) if out else None)


def test_library_argument_errors():
    D = _matrix(5, 1)
    ok = ([0, 2, 4, 1, 3], [0, 3, 5])
    assert _raw(D, 5, *ok, 2, 3, 0, 0) == _capi.ST_OK
    cases = {
        "universe below 3": (D, 2, *ok, 2, 3, 0, 0),
        "universe above the limit": (D, _capi.HOMMOLA_MAX_UNIVERSE + 1, *ok, 2, 3, 0, 0),
        "position outside": (D, 5, [0, 2, 5, 1, 3], [0, 3, 5], 2, 3, 0, 0),
        "negative position": (D, 5, [-1, 2, 4, 1, 3], [0, 3, 5], 2, 3, 0, 0),
        "unsorted set": (D, 5, [0, 4, 2, 1, 3], [0, 3, 5], 2, 3, 0, 0),
        "duplicate": (D, 5, [0, 2, 2, 1, 3], [0, 3, 5], 2, 3, 0, 0),
        "offsets go back": (D, 5, ok[0], [0, 3, 2], 2, 3, 0, 0),
        "offsets past the positions": (D, 5, ok[0], [0, 3, 6], 2, 3, 0, 0),
        "negative permutations": (D, 5, *ok, 2, -1, 0, 0),
        "negative chunk_tasks": (D, 5, *ok, 2, 3, 0, -1),
        "negative stream": (D, 5, *ok, 2, 3, -1, 0),
        "negative n_sets": (D, 5, *ok, -1, 3, 0, 0),
        "NULL sets": (D, 5, ok[0], None, 2, 3, 0, 0),
        "NULL positions": (D, 5, None, [0, 3, 5], 2, 3, 0, 0),
        "NULL matrix": (None, 5, *ok, 2, 3, 0, 0),
        "device below -1": (D, 5, *ok, 2, 3, 0, 0, -2),
        "NULL out": (D, 5, *ok, 2, 3, 0, 0, -1, False),
    }
    for what, args in cases.items():
        assert _raw(*args) == _capi.ST_ERR_ARG, what
        assert _capi.last_error(), what
    L = _capi.load()      # the tree entry refuses its own arguments before it looks at the tree
    pos, off, univ = np.array(ok[0], dtype=np.int32), np.array(ok[1], dtype=np.int64), np.arange(5, dtype=np.int64)
    rec = np.zeros((2, 4), dtype=_capi.DISPERSION_RECORD)
    bad = _capi.ctypes.c_int64(0)
    p = _capi._ptr
    assert L.st_partner_dispersion_host(None, p(univ), 2, p(pos), 5, p(off), 2, 3, 1, 0, 0, p(rec), _capi.ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert L.st_partner_dispersion_host(None, None, 5, p(pos), 5, p(off), 2, 3, 1, 0, 0, p(rec), _capi.ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert L.st_partner_dispersion_host(None, p(univ), 5, p(pos), 5, p(off), 2, 3, 1, 0, 0, p(rec), _capi.ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert "tree is NULL" in _capi.last_error()
    with pytest.raises(ValueError):
        _capi.dispersion_matrix(D, [[0, 7]], 3, 1)
    with pytest.raises(ValueError):
        _capi.dispersion_matrix(D[:4], [[0, 1]], 3, 1)
    with pytest.raises(ValueError):
        _capi.dispersion_matrix(D, [[1, 0]], 3, 1)      # the library's own check: not increasing


def _linked():
    import pandas as pd
    from suchtree_amd import SuchLinkedTrees, SuchTree, synth
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
               {"min_partners": -1}, {"max_partners": 1.5}):
        with pytest.raises(ValueError):
            slt.partner_dispersion(**kw)
    names = list(tb.leaves.keys())
    for kw in ({"sets": [[names[0], names[0]]]},                              # a repeated member
               {"sets": [[names[0], names[1]]], "universe": names[1:5]},      # a member outside the universe
               {"sets": [[names[0], names[1]]], "universe": names[:2]},       # a universe below 3
               {"sets": [[tb.root_node, tb.leaves[names[0]]]]},               # an id that is no leaf
               {"sets": [[names[0]]], "stream": -1}, {"sets": [[names[0]]], "chunk_tasks": -1}, {"sets": [[names[0]]], "stream": 1 << 31}):
        with pytest.raises(ValueError):
            tb.dispersion(**kw)
    with pytest.raises(NodeNotFoundError):
        tb.dispersion([["nobody"]])
    # no row: nothing is launched, and neither tree goes to a device
    none = slt.partner_dispersion(of="A", min_partners=5)
    assert len(none) == 0 and len(none.leaves) == 0 and none.names == [] and none.n_universe == 9
    assert len(tb.dispersion([], permutations=3)) == 0
    assert ta._dev_tree is None and tb._dev_tree is None
