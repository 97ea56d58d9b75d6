"""PERMANOVA and ANOSIM without a GPU: the host restatement behind st_group_sums_codes (device = -1) against
tests/group_reference.py with ==, each column against the Mantel sums on the group's indicator matrix, the chunk, slice
and prefix invariances, the documented known answers, pseudo-F against scipy's one-way ANOVA, R against a restatement
with scipy's ranks, the counts behind the p-value against exact fractions (with exactly tied permutations), both paths
of the weighted sums, the errors, and the plan and restatement under the address / undefined-behaviour sanitizers in a
program of their own.  The facade's results need the trees' kernels for the matrix: tests/test_gpu_group_tests.py."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import scipy.stats

import group_reference as ref
from conftest import ROOT, golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare


def _codes(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 31), 1 << 31, n * (n - 1) // 2, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 257])
def test_integers_equal_the_reference(n):
    y = _codes(n, n)
    rng = np.random.default_rng(100 + n)
    perms = 4 if n < 257 else 2
    # six labels of which 4 has no object; labels 0 and 1 once each where n allows: groups of size 1
    g = rng.choice([2, 3, 5], n)
    g[0], g[n - 1] = 0, 1
    got = _capi.group_sums_codes(y, g, 6, perms, seed=9, stream=4)
    assert got.dtype == np.int64 and got.shape == (perms + 1, 6)
    assert got.tolist() == ref.group_sums(y, g, 6, perms, 9, 4)
    assert (got[:, [0, 1, 4]] == 0).all()
    one = _capi.group_sums_codes(y, np.zeros(n, dtype=int), 1, perms, seed=9, stream=4)
    assert one.tolist() == [[sum(y.tolist())]] * (perms + 1)
    top = rng.integers(250, 256, n)
    top[0], top[1] = 254, 255
    got = _capi.group_sums_codes(y, top, 256, perms, seed=9, stream=4)
    assert got.tolist() == ref.group_sums(y, top, 256, perms, 9, 4)


def test_a_column_is_the_mantel_sum_on_the_indicator():
    n, perms, seed, stream = 65, 5, 31, 2
    y = _codes(n, 2)
    g = np.random.default_rng(3).integers(0, 4, n)
    got = _capi.group_sums_codes(y, g, 4, perms, seed, stream)
    for h in range(4):
        x = ((g[:, None] == h) & (g[None, :] == h)).astype(np.int32)
        assert _capi.mantel_ints(_capi.mantel_codes(x, y, None, perms, seed, stream)[1], "sxy") == got[:, h].tolist()


def test_chunk_slice_and_permutation_count_change_no_byte(monkeypatch):
    n, perms = 65, 9
    y = _codes(n, 4)
    g = np.random.default_rng(5).integers(0, 7, n)
    one = _capi.group_sums_codes(y, g, 7, perms, 6, 1)
    for s in (None, 1, 3, 64):
        if s:
            monkeypatch.setenv("SUCHTREE_AMD_GROUP_SLICE", str(s))
        for chunk in (1, 2, 5, 40):
            assert _capi.group_sums_codes(y, g, 7, perms, 6, 1, chunk_tasks=chunk).tobytes() == one.tobytes(), (s, chunk)
    for k in (0, 1, 4):
        assert _capi.group_sums_codes(y, g, 7, k, 6, 1).tobytes() == one[:k + 1].tobytes()


SKBIO_D = [[0, 1, 1, 4], [1, 0, 3, 2], [1, 3, 0, 3], [4, 2, 3, 0]]


def test_documented_known_answers():
    # scikit-bio's documented examples; by hand: d^2 within = 1 + 9, SS_W = 10 / 2 = 5, SS_T = 40 / 4 = 10, F = (5 / 1) / (5 / 2);
    # midranks 1.5 1.5 6 3 4.5 4.5, within 1.5 and 4.5, between mean 3.75: R = (3.75 - 3) / (6 / 2)
    f = compare.permanova(SKBIO_D, (1, 1, 2, 2), permutations=99, seed=1, device=None)
    r = compare.anosim(np.array(SKBIO_D, dtype=float), ("a", "a", "b", "b"), permutations=99, seed=1, device=None)
    assert f.statistic == 2.0 and f.r2 == 0.5 and r.statistic == 0.25 and r.r2 is None
    assert f.method == "permanova" and r.method == "anosim" and f.labels == [1, 2] and r.labels == ["a", "b"] and f.group_sizes == [2, 2]
    assert (f.n, f.n_groups, f.permutations, f.seed) == (4, 2, 99, 1) and f.shift == 26 and r.shift is None
    assert f.within_q == [1 << 26, 9 << 26] and r.within_q == [-4, 2]      # (doubled midranks minus 7)
    stat, p, n = f
    assert (stat, p, n) == (2.0, (f.n_ge + 1) / 100, 4) and f.perm_stats is None


def _relabelled(g, seed, stream, p):
    return np.asarray(g)[_capi.hommola_permutation(seed, stream, p, 0, len(g))]


def test_pseudo_f_is_the_one_way_anova_f_of_univariate_points():
    rng = np.random.default_rng(12)
    g = np.repeat([0, 1, 2], [5, 9, 16])
    pts = rng.normal(size=30) + 0.8 * g
    d = np.abs(pts[:, None] - pts[None, :])
    got = compare.permanova(d, g, permutations=40, seed=3, stream=2, keep_stats=True, device=None)
    want = scipy.stats.f_oneway(*(pts[g == h] for h in range(3)))[0]
    print("pseudo-F: observed %.6f, relative difference from f_oneway %.3e" % (want, abs(got.statistic - want) / want))
    assert abs(got.statistic - want) <= 1e-9 * want      # (the 2^-30 quantum of the codes on a well-conditioned F)
    # A relabelled F is as small as 0.01, and SS_A = SS_T - SS_W then cancels: no fixed relative bound holds.  The bound
    # per relabelling is the worst case of the fixed point instead: every code is within half a unit of d^2 2^shift, so
    # SS_T = sum / n is within e_T = (n - 1) / 4 units and SS_W = sum over g of sum_g / n_g within e_W = sum of
    # (n_g - 1) / 4, and to first order |dF| / F <= (e_T + e_W) / SS_A + e_W / SS_W; 1e-12 on top for f_oneway's own
    # rounding.  Measured: the observed F = 5.88 differs by 6.0e-10 relative; the largest relative difference of a
    # relabelled one is 4.5e-08 (at F = 0.058), its bound there 1.7e-06.
    n, unit = len(pts), math.ldexp(1.0, got.shift)
    e_t, e_w = (n - 1) / 4, sum(s - 1 for s in (5, 9, 16)) / 4
    worst = (0.0, 0.0, 0.0)
    for p in range(1, 41):
        lab = _relabelled(g, 3, 2, p)
        parts = [pts[lab == h] for h in range(3)]
        want = scipy.stats.f_oneway(*parts)[0]
        ss_w = sum(((v - v.mean()) ** 2).sum() for v in parts) * unit
        ss_a = ((pts - pts.mean()) ** 2).sum() * unit - ss_w
        bound = (e_t + e_w) / ss_a + e_w / ss_w + 1e-12
        rel = abs(got.perm_stats[p - 1] - want) / want
        worst = max(worst, (rel, want, bound))
        assert rel <= bound, (p, want, rel, bound)
    print("pseudo-F: largest relative difference over 40 relabellings %.3e at F = %.4f (bound %.3e)" % worst)
    ss_t = ((pts - pts.mean()) ** 2).sum()
    ss_w = sum(((pts[g == h] - pts[g == h].mean()) ** 2).sum() for h in range(3))
    assert abs(got.r2 - (1 - ss_w / ss_t)) <= 1e-9


def test_anosim_r_against_a_restatement_with_scipy_ranks():
    rng = np.random.default_rng(14)
    n = 23
    v = rng.integers(0, 6, n * (n - 1) // 2).astype(np.float64) / 4      # tied, with zeros of both signs
    v[v == 0.0] *= rng.choice([-1.0, 1.0], np.count_nonzero(v == 0.0))
    assert np.signbit(v[v == 0.0]).any() and not np.signbit(v[v == 0.0]).all()
    g = rng.integers(0, 3, n)
    got = compare.anosim(v, g, permutations=30, seed=8, stream=5, keep_stats=True, device=None)
    ranks = scipy.stats.rankdata(v + 0.0)
    i, j = np.tril_indices(n, -1)
    m = len(v)
    for p in range(31):
        lab = _relabelled(g, 8, 5, p)
        within = lab[i] == lab[j]
        want = (ranks[~within].mean() - ranks[within].mean()) / (m / 2)
        have = got.statistic if p == 0 else got.perm_stats[p - 1]
        assert abs(have - want) <= 1e-12, p


def _exact_counts(d2_codes, g, perms, seed, stream):
    """(n_ge of pseudo-F, ties with the observation) from exact fractions of SS_W, a plain loop over the pairs"""
    n = len(g)
    ss = []
    for p in range(perms + 1):
        lab = _relabelled(g, seed, stream, p).tolist()
        size = {h: lab.count(h) for h in set(lab)}
        ss.append(sum(Fraction(int(d2_codes[a * (a - 1) // 2 + b]), size[lab[a]]) for a in range(n) for b in range(a) if lab[a] == lab[b]))
    return sum(s <= ss[0] for s in ss[1:]), sum(s == ss[0] for s in ss[1:])


def test_n_ge_against_exact_fractions_with_unequal_sizes():
    sizes = [2, 3, 5, 7, 11, 13]
    g = np.random.default_rng(16).permutation(np.repeat(np.arange(6), sizes))
    n = len(g)
    pts = np.random.default_rng(17).normal(size=(n, 3))
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    d = (d + d.T) / 2
    got = compare.permanova(d, g, permutations=50, seed=21, stream=1, device=None)
    codes = _capi.mantel_quantise(compare.mantel_condensed(d, "d")[0] ** 2)[0]
    n_ge, _ = _exact_counts(codes, g, 50, 21, 1)
    assert got.n_ge == n_ge and got.p_value == (n_ge + 1) / 51 and math.lcm(*sizes) == 30030


def test_label_preserving_relabellings_are_counted():
    # n = 4 in two pairs: 8 of the 24 relabellings map the groups onto themselves and give T_0 again, whatever d holds
    d = np.array([[0, 0.1, 0.7, 1.3], [0.1, 0, 0.9, 1.9], [0.7, 0.9, 0, 0.3], [1.3, 1.9, 0.3, 0]])
    got = compare.permanova(d, [0, 0, 1, 1], permutations=99, seed=4, keep_stats=True, device=None)
    codes = _capi.mantel_quantise(compare.mantel_condensed(d, "d")[0] ** 2)[0]
    n_ge, ties = _exact_counts(codes, [0, 0, 1, 1], 99, 4, 0)
    assert 10 <= ties <= 60 and got.n_ge == n_ge >= ties
    assert np.count_nonzero(got.perm_stats == got.statistic) == ties
    r = compare.anosim(d, [0, 0, 1, 1], permutations=99, seed=4, keep_stats=True, device=None)
    assert np.count_nonzero(r.perm_stats == r.statistic) >= ties and r.n_ge >= ties


def test_int64_and_python_int_sums_agree():
    n = 257
    sizes = [3, 7, 11, 13, 223]
    weights = [math.lcm(*sizes) // s for s in sizes]
    assert math.lcm(*sizes) > 1 << 10 and len(sizes) * (1 << 58) * max(weights) >= 1 << 63      # (permanova takes Python ints here)
    g = np.repeat(np.arange(5), sizes)
    small = np.random.default_rng(18).integers(-1000, 1000, n * (n - 1) // 2).astype(np.int32)      # (int64 cannot overflow on these)
    sums = _capi.group_sums_codes(small, g, 5, 6, 2, 0)
    a, b = compare.group_weighted_sums(sums, weights, False), compare.group_weighted_sums(sums, weights, True)
    assert a == b == compare.group_weighted_sums(sums, weights) and all(type(t) is int for t in a)
    assert sum(t <= a[0] for t in a[1:]) == sum(t <= b[0] for t in b[1:])
    # and the whole test on real codes, where int64 would wrap: against the exact fractions
    pts = np.random.default_rng(19).normal(size=n)
    d = np.abs(pts[:, None] - pts[None, :])
    got = compare.permanova(d, g, permutations=3, seed=2, device=None)
    codes = _capi.mantel_quantise(compare.mantel_condensed(d, "d")[0] ** 2)[0]
    assert got.n_ge == _exact_counts(codes, g, 3, 2, 0)[0]
    equal = compare.permanova(d, np.arange(n) % 2, permutations=3, seed=2, device=None)      # (sizes 129, 128: Python ints too)
    assert equal.n_ge == _exact_counts(codes, np.arange(n) % 2, 3, 2, 0)[0]
    assert compare.group_weighted_sums(sums[:, :2], [1, 1]) == sums[:, :2].sum(axis=1).tolist()      # (the int64 path by itself)


def test_errors_name_the_offender():
    d = np.array(SKBIO_D, dtype=float)
    for fn in (compare.permanova, compare.anosim):
        for grouping, text in (((1, 1, 1, 1), "one group"), ((1, 2, 3, 4), "alone"), ((1, 1, 2), "3 labels for 4 objects")):
            with pytest.raises(ValueError, match=text):
                fn(d, grouping, device=None)
        bad = d.copy()
        bad[2, 1] = 5.0
        with pytest.raises(ValueError, match=r"d\[2\]\[1\]"):
            fn(bad, (1, 1, 2, 2), device=None)
        bad[2, 1] = bad[1, 2] = np.nan
        with pytest.raises(ValueError, match="not finite"):
            fn(bad, (1, 1, 2, 2), device=None)
        for kw in ({"permutations": -1}, {"seed": -1}, {"stream": -1}, {"chunk_tasks": -1}):
            with pytest.raises(ValueError):
                fn(d, (1, 1, 2, 2), device=None, **kw)
        with pytest.raises(ValueError):
            fn(d[:2, :2], (1, 2), device=None)
        big = np.zeros((300, 300))
        with pytest.raises(ValueError, match="257 groups"):
            fn(big, list(range(257)) + [0] * 43, device=None)
    fresh = compare.permanova(d, (1, 1, 2, 2), permutations=9, device=None)
    again = compare.permanova(d, (1, 1, 2, 2), permutations=9, seed=fresh.seed, device=None)
    assert fresh.seed is not None and (fresh.n_ge, fresh.statistic) == (again.n_ge, again.statistic)
    for g, text in (([0, 1, 2, 300, 0], "group\\[3\\] = 300"), ([0, -1, 2, 0, 0], "group\\[1\\] = -1")):
        with pytest.raises(ValueError, match=text):
            _capi.group_sums_codes(np.zeros(10, dtype=np.int32), g, 3, 1)
    with pytest.raises(ValueError, match="10 pairs of 5 objects"):
        _capi.group_sums_codes(np.zeros(9, dtype=np.int32), [0] * 5, 1, 1)


def _raw(y, g, n, n_groups=3, perms=1, stream=0, chunk=0, device=-1, out=True):
    L = _capi.load()
    y = None if y is None else np.ascontiguousarray(y, dtype=np.int32)
    g = None if g is None else np.ascontiguousarray(g, dtype=np.uint8)
    res = np.zeros((max(min(perms, 16), 0) + 1, 256), dtype=np.int64)
    p = _capi._ptr
    return L.st_group_sums_codes(device, p(y), n, p(g), n_groups, perms, 1, stream, chunk, p(res) if out else None)


def test_library_argument_errors_in_the_stated_order():
    y, g = _codes(5, 1), np.array([0, 1, 2, 1, 0])
    E = _capi.ST_ERR_ARG
    for args, text in (((None, None, 2, 0, -1, -1, -1, -2, False), "a universe of 2 positions"),
                       ((None, None, 16385, 0, -1, -1, -1, -2, False), "a universe of 16385 positions"),
                       ((None, None, 5, 0, -1, -1, -1, -2, False), "permutations < 0"),
                       ((None, None, 5, 0, 1, -1, -1, -2, False), "chunk_tasks < 0"),
                       ((None, None, 5, 0, 1, -1, 0, -2, False), "stream < 0"),
                       ((None, None, 5, 0, 1 << 31, 0, 0, -2, False), "more than 2^31 - 1 permutations"),
                       ((None, None, 5, 0, 1, 0, 0, -2, False), "0 groups: 1 to 256"),
                       ((None, None, 5, 257, 1, 0, 0, -2, False), "257 groups: 1 to 256"),
                       ((None, g, 5, 3, 1, 0, 0, -2, False), "y or group is NULL"),
                       ((y, None, 5, 3, 1, 0, 0, -2, False), "y or group is NULL"),
                       ((y, g, 5, 3, 1, 0, 0, -2, False), "out is NULL"),
                       ((y, g, 5, 2, 1, 0, 0, -2, True), "group[2] = 2 of 2 groups"),
                       ((y, g, 5, 3, 1, 0, 0, -2, True), "device must be -1")):
        assert _raw(*args) == E and text in _capi.last_error(), text
    assert _raw(y, g, 5) == _capi.ST_OK


def test_facade_errors_raised_before_any_upload():
    d = golden_path("gopher_louse")
    ta, tb = SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree")
    slt = SuchLinkedTrees(ta, tb, pd.read_csv(d + "/links.csv", index_col=0))
    inner = [int(v) for v in ta.get_internal_nodes() if int(v) != ta.root_node]
    child = next(v for v in inner if int(ta._flat.parent[v]) in inner)
    names = list(ta.leaves.keys())
    halves = {name: k % 2 for k, name in enumerate(names)}
    with pytest.raises(ValueError, match="clades %d and %d overlap" % (int(ta._flat.parent[child]), child)):
        slt.partner_group_differences(groups=[int(ta._flat.parent[child]), child])
    for kw in ({"of": "C"}, {"measure": "jaccard"}, {"test": "permdisp"}, {"permutations": -1}, {"seed": -1}, {"chunk_tasks": -1}, {"min_partners": -1},
               {"groups": None}, {"groups": {names[0]: 0, names[1]: 1}}, {"groups": {name: 0 for name in names}},
               {"groups": {name: k for k, name in enumerate(names)}}):
        with pytest.raises(ValueError):
            slt.partner_group_differences(**dict({"groups": halves}, **kw))
    assert ta._dev_tree is None and tb._dev_tree is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_group_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_group")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_group.cpp"), os.path.join(csrc, "group_plan.cpp"),
                           os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize group ok" in out.stdout
