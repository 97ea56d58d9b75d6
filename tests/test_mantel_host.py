"""The Mantel and partial Mantel tests without a GPU: the host restatement behind st_mantel_codes (device = -1) against
tests/mantel_reference.py with ==, the quantiser, the rank codes, the coefficients against scipy, the counts behind the
p-value against a plain loop (with exactly tied permutations), the prefix property, the input forms, the errors, and the
plan and restatement under the address / undefined-behaviour sanitizers in a program of their own."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
import scipy.stats

import mantel_reference as ref
from conftest import ROOT, golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare


def _codes(n, seed, wide=True):
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    lo, hi = (-(1 << 31), 1 << 31) if wide else (-50, 50)
    draw = lambda k: rng.integers(lo, hi, k, dtype=np.int64).astype(np.int32)      # noqa: E731
    x = ref.square(draw(m), n)
    x[np.arange(n), np.arange(n)] = draw(n)      # (ignored)
    return x, draw(m), draw(m)


@pytest.mark.parametrize("n", [3, 4, 64, 65, 257])
def test_integers_equal_the_reference(n):
    x, y, z = _codes(n, n)
    perms = 3 if n > 100 else 6
    for third in (None, z):
        mom, rec = _capi.mantel_codes(x, y, third, perms, seed=17, stream=4)
        assert mom == ref.moments(x, y, third)
        want = ref.records(x, y, third, perms, 17, 4)
        assert list(zip(_capi.mantel_ints(rec, "sxy"), _capi.mantel_ints(rec, "sxz"))) == want
    # chunk_tasks changes the plan, never a record
    assert _capi.mantel_codes(x, y, z, perms, 17, 4, -1, 2)[1].tobytes() == rec.tobytes()


def test_carry_past_64_bits():
    n, top = 65, (1 << 31) - 1
    m = n * (n - 1) // 2
    x = np.full((n, n), top, dtype=np.int32)
    for sign in (1, -1):
        y = np.full(m, sign * top, dtype=np.int32)
        mom, rec = _capi.mantel_codes(x, y, y, 2, seed=1)
        want = sign * m * top * top
        assert abs(want) > 1 << 63 and m == 2080
        assert _capi.mantel_ints(rec, "sxy") == [want] * 3 and _capi.mantel_ints(rec, "sxz") == [want] * 3
        assert mom["sxx"] == m * top * top and mom["syz"] == m * top * top and mom["sy"] == sign * m * top


def test_quantiser():
    rng = np.random.default_rng(2)
    for v in (rng.random(50) * 7.3, rng.normal(size=40) * 1e-12, rng.normal(size=40) * 1e15, np.array([0.0, -0.0]),
              np.array([np.nextafter(2.0, 0.0), 0.3]), np.array([-5.0, 1.0, 2.5])):
        q, shift = _capi.mantel_quantise(v)
        want, want_shift = ref.quantise(v)
        assert shift == want_shift and q.tolist() == want
        top = max(abs(t) for t in want)
        assert (1 << 30) <= top < (1 << 31) or not v.any()
        q4, s4 = _capi.mantel_quantise(v, shift - 4)      # a caller's shift
        assert s4 == shift - 4 and q4.tolist() == ref.quantise(v, shift - 4)[0]
    with pytest.raises(ValueError, match="2\\^31"):
        _capi.mantel_quantise(np.array([1.0, 3.0]), 30)
    with pytest.raises(ValueError, match="v\\[2\\]"):
        _capi.mantel_quantise(np.array([1.0, 3.0, np.nan]))
    with pytest.raises(ValueError, match="v\\[0\\]"):
        _capi.mantel_quantise(np.array([-np.inf, 3.0, np.nan]))


def test_rank_codes_with_ties_and_signed_zeros():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.integers(0, 6, 40) / 4.0, [0.0, -0.0, -0.0, 0.0, -1.5, -1.5], rng.random(20)])
    rng.shuffle(v)
    m = len(v)
    got = compare.mantel_rank_codes(v)
    want = 2 * scipy.stats.rankdata(v, "average") - (m + 1)
    assert got.dtype == np.int32 and (got == want).all() and got.tolist() == ref.rank_codes(v)
    zeros = np.flatnonzero(v == 0.0)
    assert len(set(got[zeros].tolist())) == 1 and np.signbit(v[zeros]).any() and not np.signbit(v[zeros]).all()


def _patristic(tree, leaves):
    """float64 distances between the named leaves, from the flat arrays on the host"""
    parent, dist = np.asarray(tree._flat.parent), np.asarray(tree._flat.distance, dtype=np.float64)
    paths = []
    for name in leaves:
        v, path = int(tree.leaves[name]), {}
        d = 0.0
        while v != -1:
            path[v] = d
            d += dist[v]
            v = int(parent[v])
        paths.append(path)
    n = len(leaves)
    D = np.zeros((n, n))
    for a in range(n):
        for b in range(a):
            D[a, b] = D[b, a] = min(paths[a][v] + paths[b][v] for v in paths[a] if v in paths[b])
    return D


def _linked(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links


@pytest.fixture(scope="module")
def fixtures():
    """name -> (x, y, z): the hosts' tree distances, the tree distances of each host's first guest, and a third matrix --
    for gopher / louse and fish / worm -- and one seeded random triple"""
    out = {}
    for which in ("gopher_louse", "fish_worm"):
        ta, tb, links = _linked(which)
        hosts = [h for h in links.index if links.loc[h].sum() > 0]
        x = _patristic(ta, hosts)
        y = _patristic(tb, [links.columns[np.flatnonzero(links.loc[h].values > 0)[0]] for h in hosts])
        out[which] = (x, y, np.sqrt(x + y.T))
    rng = np.random.default_rng(8)
    a = rng.random((40, 40))
    b = a + rng.normal(size=(40, 40)) * 0.3
    c = rng.random((40, 40))
    out["random"] = tuple(np.triu(t, 1) + np.triu(t, 1).T for t in (a, b, c))
    return out


def test_spearman_r_against_scipy(fixtures):
    for name, (x, y, _) in fixtures.items():
        got = compare.mantel(x, y, method="spearman", permutations=0, seed=0, device=None)
        want = scipy.stats.spearmanr(ref.condensed(x), ref.condensed(y))[0]
        assert abs(got.corr_coeff - want) <= 1e-12, name
        assert got.shift_x is None and got.n_pairs == len(ref.condensed(x))


# The largest |corr_coeff - scipy.stats.pearsonr| over the three fixtures, measured on the CPU of the development machine
# (profiles/mantel_r25.log): 1.3e-10 (gopher / louse 5.6e-16, fish / worm 1.3e-10, random 2.0e-12).  It is the 31-bit
# fixed point, up to half a unit in 2^30 a value, not the summation, which is exact.  The bound is 16 times that, for another libm.
PEARSON_MEASURED = 1.3e-10


def test_pearson_r_against_scipy(fixtures):
    worst = 0.0
    for name, (x, y, _) in fixtures.items():
        got = compare.mantel(x, y, permutations=0, seed=0, device=None)
        want = scipy.stats.pearsonr(ref.condensed(x), ref.condensed(y))[0]
        print("pearson |difference| %s: %.3e" % (name, abs(got.corr_coeff - want)))
        worst = max(worst, abs(got.corr_coeff - want))
    print("pearson largest |difference|: %.3e" % worst)
    assert worst <= 16 * PEARSON_MEASURED


def test_partial_r_against_the_textbook_formula(fixtures):
    for name, (x, y, z) in fixtures.items():
        got = compare.mantel(x, y, z, permutations=0, seed=0, device=None)
        r = lambda a, b: scipy.stats.pearsonr(ref.condensed(a), ref.condensed(b))[0]      # noqa: E731
        want = (r(x, y) - r(x, z) * r(y, z)) / math.sqrt((1 - r(x, z) ** 2) * (1 - r(y, z) ** 2))
        assert abs(got.corr_coeff - want) <= 16 * PEARSON_MEASURED * 4, name      # (three coefficients and a quotient)
        assert got.partial and got.sxz is not None and got.shift_z is not None


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_p_value_against_a_plain_loop(fixtures, method):
    x, y, _ = fixtures["gopher_louse"]
    perms, seed, stream = 60, 23, 2
    if method == "pearson":
        cx, cy = ref.quantise(ref.condensed(x))[0], ref.quantise(ref.condensed(y))[0]
    else:
        cx, cy = ref.rank_codes(ref.condensed(x)), ref.rank_codes(ref.condensed(y))
    r, n_ge, n_le, n_abs_ge = ref.simple_test(ref.square(cx, len(x), np.int64), cy, perms, seed, stream)
    for alternative, count in (("greater", n_ge), ("less", n_le), ("two-sided", n_abs_ge)):
        got = compare.mantel(x, y, method=method, permutations=perms, seed=seed, stream=stream, alternative=alternative, device=None)
        assert (got.n_ge, got.n_le, got.n_abs_ge) == (n_ge, n_le, n_abs_ge)
        assert got.p_value == ref.p_value(count, perms) and got.corr_coeff == r
        assert tuple(got) == (got.corr_coeff, got.p_value, len(x))


def test_an_exactly_tied_permutation_is_counted():
    # two groups of three: x is 0 within a group and 1 between, so 72 of the 720 relabellings leave x as it is and give
    # the observed sum again, whatever y holds -- values that a float sum would not reproduce to the last bit
    n, perms, seed = 6, 200, 5
    x = np.array([[0.0 if (i < 3) == (j < 3) else 1.0 for j in range(n)] for i in range(n)])
    y = ref.square(np.array([0.1, 0.2, 0.3, 0.7, 1.1, 1.3, 0.9, 1.7, 1.9, 0.15, 2.3, 2.9, 3.1, 0.25, 0.35]), n)
    cx, cy = ref.quantise(ref.condensed(x))[0], ref.quantise(ref.condensed(y))[0]
    rec = ref.records(ref.square(cx, n, np.int64), cy, None, perms, seed)
    ties = sum(s == rec[0] for s in rec[1:])
    assert 5 <= ties < perms // 2
    got = compare.mantel(x, y, permutations=perms, seed=seed, alternative="greater", keep_stats=True, device=None)
    assert got.n_ge + got.n_le - perms == ties      # (counted on both sides)
    assert got.n_ge == sum(s >= rec[0] for s in rec[1:]) and got.p_value == (got.n_ge + 1) / (perms + 1)
    assert np.count_nonzero(got.perm_stats == got.corr_coeff) == ties


def test_prefix_property_and_input_forms(fixtures):
    x, y, z = fixtures["fish_worm"]
    long = compare.mantel(x, y, z, permutations=40, seed=9, keep_stats=True, device=None)
    short = compare.mantel(x, y, z, permutations=12, seed=9, keep_stats=True, device=None)
    assert long.perm_stats[:12].tobytes() == short.perm_stats.tobytes() and long.corr_coeff == short.corr_coeff
    simple = compare.mantel(x, y, permutations=40, seed=9, keep_stats=True, device=None)
    assert simple.perm_stats[:12].tobytes() == compare.mantel(x, y, permutations=12, seed=9, keep_stats=True, device=None).perm_stats.tobytes()
    flat = compare.mantel(ref.condensed(x), ref.condensed(y), ref.condensed(z), permutations=40, seed=9, keep_stats=True, device=None)
    mixed = compare.mantel(x, ref.condensed(y), z, permutations=40, seed=9, keep_stats=True, device=None)
    for other in (flat, mixed):
        assert other.perm_stats.tobytes() == long.perm_stats.tobytes() and other.sxy == long.sxy and other.p_value == long.p_value
    # the diagonal is ignored
    xd = x + np.diag(np.arange(len(x)) + 1.0)
    assert compare.mantel(xd, y, z, permutations=12, seed=9, device=None).sxy == short.sxy
    # a drawn seed is reported and repeats the run
    drawn = compare.mantel(x, y, permutations=12, device=None)
    again = compare.mantel(x, y, permutations=12, seed=drawn.seed, device=None)
    assert (drawn.n_ge, drawn.n_le, drawn.n_abs_ge) == (again.n_ge, again.n_le, again.n_abs_ge)


def test_constant_matrix_gives_nan(fixtures):
    x, y, z = fixtures["gopher_louse"]
    flat = np.ones_like(x)
    for args in ((flat, y, None), (x, flat, None), (x, y, flat), (flat, y, z)):
        got = compare.mantel(*args, permutations=5, seed=1, device=None)
        assert math.isnan(got.corr_coeff) and math.isnan(got.p_value)


def test_errors_name_the_offender(fixtures):
    x, y, _ = fixtures["gopher_louse"]
    bad = y.copy()
    bad[4, 2] += 0.5
    with pytest.raises(ValueError, match=r"y is not symmetric: y\[4\]\[2\]"):
        compare.mantel(x, bad, device=None)
    bad = y.copy()
    bad[3, 1] = bad[1, 3] = np.nan
    with pytest.raises(ValueError, match=r"y\[1\]\[3\].*not finite|y\[3\]\[1\].*not finite"):
        compare.mantel(x, bad, device=None)
    bad = ref.condensed(x).copy()
    bad[7] = np.inf
    with pytest.raises(ValueError, match=r"x\[7\]"):
        compare.mantel(bad, y, device=None)
    with pytest.raises(ValueError, match="n = 2 objects"):
        compare.mantel(np.zeros((2, 2)), np.zeros((2, 2)), device=None)
    with pytest.raises(ValueError, match="n = 16385 objects"):
        compare.mantel(np.broadcast_to(np.float64(0.0), (16385, 16385)), y, device=None)
    with pytest.raises(ValueError, match="y has 4 objects, x has %d" % len(x)):
        compare.mantel(x, np.zeros(6), device=None)
    with pytest.raises(ValueError, match="pairs of any n"):
        compare.mantel(x, np.zeros(7), device=None)
    for kw in ({"method": "kendall"}, {"alternative": "both"}, {"permutations": -1}, {"permutations": 2.5}, {"seed": -1}, {"stream": -1},
               {"chunk_tasks": -1}, {"stream": 1 << 31}):
        with pytest.raises(ValueError):
            compare.mantel(x, y, device=None, **kw)


def _raw(x, y, n, perms=1, stream=0, chunk=0, device=-1, moments=True, out=True):
    L = _capi.load()
    x = None if x is None else np.ascontiguousarray(x, dtype=np.int32)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.int32)
    rec = np.zeros(max(min(perms, 16), 0) + 1, dtype=_capi.MANTEL_SUMS)
    mom = _capi.MantelMoments()
    p = _capi._ptr
    return L.st_mantel_codes(device, p(x), p(y), None, n, perms, 1, stream, chunk, ctypes.byref(mom) if moments else None, p(rec) if out else None)


def test_library_argument_errors_in_the_stated_order():
    x, y, _ = _codes(5, 1)
    E = _capi.ST_ERR_ARG
    for args, text in (((None, None, 2, -1, -1, -1, -2, False, False), "a universe of 2 positions"),
                       ((None, None, 16385, -1, -1, -1, -2, False, False), "a universe of 16385 positions"),
                       ((None, None, 5, -1, -1, -1, -2, False, False), "permutations < 0"),
                       ((None, None, 5, 1, -1, -1, -2, False, False), "chunk_tasks < 0"),
                       ((None, None, 5, 1, -1, 0, -2, False, False), "stream < 0"),
                       ((None, None, 5, 1 << 31, 0, 0, -2, False, False), "more than 2^31 - 1 permutations"),
                       ((None, y, 5, 1, 0, 0, -2, False, False), "x_sq or y is NULL"),
                       ((x, None, 5, 1, 0, 0, -2, False, False), "x_sq or y is NULL"),
                       ((x, y, 5, 1, 0, 0, -2, False, True), "moments or out is NULL"),
                       ((x, y, 5, 1, 0, 0, -2, True, False), "moments or out is NULL"),
                       ((x, y, 5, 1, 0, 0, -2, True, True), "device must be -1")):
        assert _raw(*args) == E and text in _capi.last_error(), text
    bad = x.copy()
    bad[3, 1] ^= 1
    bad[4, 0] ^= 1
    assert _raw(bad, y, 5) == E and "x_sq is not symmetric: x_sq[0][4]" in _capi.last_error()
    assert _raw(x, y, 5) == _capi.ST_OK


def test_facade_errors_raised_before_any_upload():
    ta, tb, links = _linked("gopher_louse")
    slt = SuchLinkedTrees(ta, tb, links)
    for kw in ({"of": "C"}, {"measure": "jaccard"}, {"method": "kendall"}, {"alternative": "both"}, {"permutations": -1}, {"seed": -1},
               {"pool": "all"}, {"min_partners": -1}, {"chunk_tasks": -1}, {"min_partners": 3}):      # (the last: fewer than 3 rows)
        with pytest.raises(ValueError):
            slt.phylosymbiosis(**kw)
    names = list(ta.leaves.keys())
    y = np.zeros((len(names), len(names)))
    for kw in ({"leaves": names[:2], "y": np.zeros(1)}, {"leaves": names[:4] + names[:1], "y": np.zeros(10)}, {"leaves": names, "y": np.zeros(6)},
               {"leaves": names, "y": y, "z": np.zeros(6)}, {"leaves": [ta.root_node, 0, 1], "y": np.zeros(3)}):
        with pytest.raises(ValueError):
            ta.mantel(**kw)
    assert ta._dev_tree is None and tb._dev_tree is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_mantel_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_mantel")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_mantel.cpp"), os.path.join(csrc, "mantel_plan.cpp"),
                           os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize mantel ok" in out.stdout
