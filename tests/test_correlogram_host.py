"""The Mantel correlogram without a GPU: the host restatement behind st_class_sums_codes (device = -1) against a numpy
restatement written from the definition, compared by tobytes(); the row sums; the chunk, slice and prefix invariances;
every argument error in its order; compare.mantel_correlogram against compare.mantel on each class's indicator (the counts
exactly, the sign flipped) and against numpy.corrcoef; the class edges, Sturges' default, the cutoff, the corrections
against a restatement, the NaN rows, the class limit; and the plan and restatement under the address /
undefined-behaviour sanitizers in a program of their own.  The facades need the trees' kernels for the matrices:
tests/test_gpu_correlogram.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from suchtree_amd import _capi, compare

NONE = _capi.CLASS_NONE


def _codes(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 31), 1 << 31, n * (n - 1) // 2, dtype=np.int64).astype(np.int32)


def _restate(y, cls, n_classes, perms, seed, stream):
    """out[p][c] from the definition: the y values under the mask cls_sq[np.ix_(s, s)] == c, condensed"""
    n = (1 + math.isqrt(8 * len(y) + 1)) // 2
    i, j = np.tril_indices(n, -1)
    cls_sq = np.full((n, n), NONE, dtype=np.uint8)
    cls_sq[i, j] = cls_sq[j, i] = cls
    out = np.zeros((perms + 1, n_classes), dtype=np.int64)
    for p in range(perms + 1):
        s = compare.hommola_permutation(seed, stream, p, 0, n)
        relabelled = cls_sq[np.ix_(s, s)][i, j]
        for c in range(n_classes):
            out[p, c] = y[relabelled == c].sum(dtype=np.int64)
    return out


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 66, 130])
@pytest.mark.parametrize("n_classes", [1, 2, 64])
def test_integers_equal_the_definition(n, n_classes):
    y = _codes(n, n)
    cls = np.random.default_rng(100 * n + n_classes).integers(0, n_classes, len(y)).astype(np.uint8)
    got = _capi.class_sums_codes(y, cls, n_classes, 4, seed=9, stream=4)
    assert got.dtype == np.int64 and got.shape == (5, n_classes)
    assert got.tobytes() == _restate(y, cls, n_classes, 4, 9, 4).tobytes()
    # no pair in none: every row sums to sum(y)
    assert got.sum(axis=1).tolist() == [int(y.sum(dtype=np.int64))] * 5


@pytest.mark.parametrize("n", [5, 64, 66])
def test_pairs_in_no_class(n):
    y = _codes(n, 7 * n)
    rng = np.random.default_rng(n)
    cls = rng.integers(60, 64, len(y)).astype(np.uint8)      # (class 63 beside ST_CLASS_NONE)
    cls[rng.random(len(y)) < 0.4] = NONE
    cls[:2] = (63, NONE)
    got = _capi.class_sums_codes(y, cls, 64, 3, seed=2, stream=1)
    assert got.tobytes() == _restate(y, cls, 64, 3, 2, 1).tobytes()
    assert (got[:, :60] == 0).all() and got[0, 63] != 0
    assert (got.sum(axis=1) != int(y.sum(dtype=np.int64))).any()
    none = _capi.class_sums_codes(y, np.full(len(y), NONE, dtype=np.uint8), 3, 3, seed=2, stream=1)
    assert none.shape == (4, 3) and (none == 0).all()


def test_chunk_slice_and_permutation_count_change_no_byte(monkeypatch):
    n, perms = 65, 9
    y = _codes(n, 4)
    cls = np.random.default_rng(5).integers(0, 7, len(y)).astype(np.uint8)
    one = _capi.class_sums_codes(y, cls, 7, perms, 6, 1)
    for s in (None, 1, 3, 64):
        if s:
            monkeypatch.setenv("SUCHTREE_AMD_CLASS_SLICE", str(s))
        for chunk in (1, 2, 5, 40):
            assert _capi.class_sums_codes(y, cls, 7, perms, 6, 1, chunk_tasks=chunk).tobytes() == one.tobytes(), (s, chunk)
    for k in (0, 1, 4):
        assert _capi.class_sums_codes(y, cls, 7, k, 6, 1).tobytes() == one[:k + 1].tobytes()


def _raw(y, c, n, n_classes=3, perms=1, stream=0, chunk=0, device=-1, out=True):
    L = _capi.load()
    y = None if y is None else np.ascontiguousarray(y, dtype=np.int32)
    c = None if c is None else np.ascontiguousarray(c, dtype=np.uint8)
    res = np.zeros((max(min(perms, 16), 0) + 1, 64), dtype=np.int64)
    p = _capi._ptr
    return L.st_class_sums_codes(device, p(y), p(c), n, n_classes, perms, 1, stream, chunk, p(res) if out else None)


def test_library_argument_errors_in_the_stated_order():
    y, c = _codes(5, 1), np.array([0, 1, NONE, 1, 2, 254, 1, 0, 0, 1])
    ok = np.array([0, 1, NONE, 1, 2, 2, 1, 0, 0, 1])
    E = _capi.ST_ERR_ARG
    for args, text in (((None, None, 2, 0, -1, -1, -1, -2, False), "a universe of 2 positions"),
                       ((None, None, 16385, 0, -1, -1, -1, -2, False), "a universe of 16385 positions"),
                       ((None, None, 5, 0, -1, -1, -1, -2, False), "permutations < 0"),
                       ((None, None, 5, 0, 1, -1, -1, -2, False), "chunk_tasks < 0"),
                       ((None, None, 5, 0, 1, -1, 0, -2, False), "stream < 0"),
                       ((None, None, 5, 0, 1 << 31, 0, 0, -2, False), "more than 2^31 - 1 permutations"),
                       ((None, None, 5, 0, 1, 0, 0, -2, False), "0 classes: 1 to 64"),
                       ((None, None, 5, 65, 1, 0, 0, -2, False), "65 classes: 1 to 64"),
                       ((None, c, 5, 3, 1, 0, 0, -2, False), "y or cls is NULL"),
                       ((y, None, 5, 3, 1, 0, 0, -2, False), "y or cls is NULL"),
                       ((y, c, 5, 3, 1, 0, 0, -2, False), "out is NULL"),
                       ((y, c, 5, 2, 1, 0, 0, -2, True), "cls[4] = 2 of 2 classes"),
                       ((y, c, 5, 3, 1, 0, 0, -2, True), "cls[5] = 254 of 3 classes"),
                       ((y, ok, 5, 3, 1, 0, 0, -2, True), "device must be -1")):
        assert _raw(*args) == E and text in _capi.last_error(), text
    assert _raw(y, ok, 5) == _capi.ST_OK
    with pytest.raises(ValueError, match=r"cls\[1\] = 256"):
        _capi.class_sums_codes(y, [0, 256, 0, 0, 0, 0, 0, 0, 0, 0], 1, 1)
    with pytest.raises(ValueError, match="one length"):
        _capi.class_sums_codes(y, [0] * 9, 1, 1)
    with pytest.raises(ValueError, match="not the triangle"):
        _capi.class_sums_codes(y[:9], [0] * 9, 1, 1)


def _points(n, seed):
    """(x, y): condensed distances of n random points of the plane, and a y that follows x at short range"""
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 2))
    i, j = np.tril_indices(n, -1)
    x = np.sqrt(((pts[i] - pts[j]) ** 2).sum(axis=1))
    return x, np.minimum(x, 1.0) + 0.3 * rng.random(len(x))


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_each_class_is_the_mantel_test_of_its_indicator(method):
    n, perms, seed = 66, 49, 17
    x, y = _points(n, 3)
    got = compare.mantel_correlogram(x, y, n_classes=6, cutoff=False, method=method, permutations=perms, seed=seed, keep_stats=True, device=None)
    assert len(got) == 6 and got.tested.all() and got.n == n and got.method == method and (got.seed, got.stream, got.permutations) == (seed, 0, perms)
    assert got.n_pairs.sum() == len(x) and (got.n_pairs > 0).all()
    cls = compare.mantel_classes(x, got.breaks)
    ranks = compare.mantel_rank_codes(y).astype(np.float64)
    for c in range(6):
        indicator = (cls == c).astype(np.float64)
        one = compare.mantel(indicator, y, method="pearson", permutations=perms, seed=seed, keep_stats=True, device=None)
        if method == "pearson":      # (the sign is flipped: r_c falls as the sum of the class rises)
            assert (int(got.n_ge[c]), int(got.n_le[c])) == (one.n_le, one.n_ge)
            assert np.abs(got.perm_stats[:, c] + one.perm_stats).max() <= 1e-9
        want = -np.corrcoef(indicator, y if method == "pearson" else ranks)[0, 1]
        # float64 rounding over 2145 pairs stays below 1e-12 and the 2^-31 quantum of the codes moves r by less; 1e-9 leaves
        # three orders of magnitude, and a wrong class count or sign is off by far more
        assert abs(got.corr_coeff[c] - want) <= 1e-9, (c, got.corr_coeff[c], want)
        count = got.n_ge[c] if got.corr_coeff[c] >= 0 else got.n_le[c]
        assert got.p_value[c] == (count + 1) / (perms + 1)
        row = got.row(c)
        assert row["n_pairs"] == got.n_pairs[c] and row["lower"] == got.breaks[c] and row["upper"] == got.breaks[c + 1]
    assert got.corr_coeff[0] > 0 and got.p_value[0] == 1 / (perms + 1)      # (y follows x at short range)
    sums = _capi.class_sums_codes(_capi.mantel_quantise(y)[0] if method == "pearson" else compare.mantel_rank_codes(y), cls, 6, perms, seed, 0)
    assert got.sums_q.tolist() == sums[0].tolist()
    assert got.n_ge.tolist() == (sums[1:] <= sums[0]).sum(axis=0).tolist() and got.n_le.tolist() == (sums[1:] >= sums[0]).sum(axis=0).tolist()
    frame = got.to_dataframe()
    assert len(frame) == 6 and list(frame.columns[:3]) == ["lower", "upper", "class_mid"] and frame["n_ge"].tolist() == got.n_ge.tolist()
    again = compare.mantel_correlogram(x, y, n_classes=6, cutoff=False, method=method, permutations=perms, seed=seed, device=None)
    assert again.perm_stats is None and again.p_corrected.tolist() == got.p_corrected.tolist()


def test_class_edges():
    breaks = [1.0, 2.0, 3.0, 5.0]
    x = np.array([0.999, 1.0, 1.5, 2.0, 2.999, 3.0, 5.0, 5.001, -1.0, 4.0])
    # a value on an inner edge goes up, the last edge is closed, values outside are in no class
    assert compare.mantel_classes(x, breaks).tolist() == [NONE, 0, 0, 1, 1, 2, 2, NONE, NONE, 2]
    got = compare.mantel_correlogram(x, np.arange(10.0), breaks=breaks, cutoff=False, permutations=9, seed=1, device=None)
    assert got.n_pairs.tolist() == [2, 2, 3] and got.breaks.tolist() == breaks and got.class_mid.tolist() == [1.5, 2.5, 4.0]
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="breaks"):
            compare.mantel_correlogram(x, np.arange(10.0), breaks=bad, device=None)
    with pytest.raises(ValueError, match="breaks give 3 classes"):
        compare.mantel_correlogram(x, np.arange(10.0), breaks=breaks, n_classes=4, device=None)


def test_sturges_default_and_equal_widths():
    for n in (5, 10, 23):
        x, y = _points(n, n)
        m = n * (n - 1) // 2
        got = compare.mantel_correlogram(x, y, permutations=3, seed=1, device=None)
        K = math.ceil(1 + math.log2(m))
        assert len(got) == K == {10: 5, 45: 7, 253: 9}[m]
        assert got.breaks.tolist() == np.linspace(x.min(), x.max(), K + 1).tolist() and got.n_pairs.sum() == m
    assert len(compare.mantel_correlogram(x, y, n_classes=4, permutations=3, seed=1, device=None)) == 4
    with pytest.raises(ValueError, match="constant"):
        compare.mantel_correlogram(np.ones(10), np.arange(10.0), device=None)


def test_cutoff_between_two_edges():
    # nine points on a line at 0 .. 8: the largest distance of the middle one is 4, of every other one more
    pos = np.arange(9.0)
    x = np.abs(pos[:, None] - pos[None, :])
    y = np.random.default_rng(4).random((9, 9))
    y = y + y.T
    breaks = [0.0, 1.5, 3.5, 5.5, 8.0]
    cut = compare.mantel_correlogram(x, y, breaks=breaks, permutations=19, seed=2, device=None)
    assert cut.tested.tolist() == [True, True, False, False]
    assert np.isnan(cut.p_value[2:]).all() and np.isnan(cut.p_corrected[2:]).all() and np.isfinite(cut.corr_coeff).all()
    assert np.isfinite(cut.p_value[:2]).all()
    at_edge = compare.mantel_correlogram(x, y, breaks=[0.0, 1.5, 4.0, 5.5, 8.0], permutations=19, seed=2, device=None)
    assert at_edge.tested.tolist() == [True, True, False, False]      # (an upper edge at the cut is tested)
    every = compare.mantel_correlogram(x, y, breaks=breaks, cutoff=False, permutations=19, seed=2, device=None)
    assert every.tested.all() and every.p_value[:2].tolist() == cut.p_value[:2].tolist()
    assert every.sums_q.tolist() == cut.sums_q.tolist() and every.n_ge.tolist() == cut.n_ge.tolist()
    # progressive: the first two classes are corrected alike with or without the classes beyond
    assert every.p_corrected[:2].tolist() == cut.p_corrected[:2].tolist()


def _adjust(p, correction, progressive):
    """the restatement: class k within the first k + 1 (progressive) or within all"""
    def within(q):
        t = len(q)
        if correction == "bonferroni":
            return [min(1.0, t * v) for v in q]
        order = sorted(range(t), key=lambda k: q[k])
        out, top = [0.0] * t, 0.0
        for rank, k in enumerate(order):
            top = max(top, min(1.0, (t - rank) * q[k]))
            out[k] = top
        return out
    return [within(p[:k + 1])[k] for k in range(len(p))] if progressive else within(p)


def test_corrections_against_a_restatement():
    p = [0.01, 0.04, 0.03, 0.005, 0.5, 0.02, 0.9]
    for correction in ("holm", "bonferroni"):
        for progressive in (True, False):
            assert compare.mantel_adjust(p, correction, progressive).tolist() == _adjust(p, correction, progressive), (correction, progressive)
    assert compare.mantel_adjust(p, None, True).tolist() == p
    # by hand: Holm within all seven; progressive Bonferroni multiplies the k-th value by k
    assert compare.mantel_adjust(p, "holm", False).tolist() == [0.06, 0.12, 0.12, 0.035, 1.0, 0.1, 1.0]
    assert compare.mantel_adjust(p, "bonferroni", True).tolist() == [0.01, 0.08, 0.09, 0.02, 1.0, 0.12, 1.0]
    with pytest.raises(ValueError, match="correction"):
        compare.mantel_adjust(p, "fdr")
    x, y = _points(30, 8)
    for correction in ("holm", "bonferroni", None):
        for progressive in (True, False):
            got = compare.mantel_correlogram(x, y, n_classes=8, permutations=29, seed=3, correction=correction, progressive=progressive, device=None)
            assert 0 < got.tested.sum() < 8
            want = _adjust(got.p_value[got.tested].tolist(), correction, progressive) if correction else got.p_value[got.tested].tolist()
            assert got.p_corrected[got.tested].tolist() == want and np.isnan(got.p_corrected[~got.tested]).all()


def test_nan_rows():
    x, y = _points(12, 5)
    lo, hi = x.min(), x.max()
    # an empty class between two edges that no distance reaches, and one class that holds every pair
    gap = compare.mantel_correlogram(x, y, breaks=[lo, hi + 1.0, hi + 2.0], cutoff=False, permutations=9, seed=1, device=None)
    assert gap.n_pairs.tolist() == [len(x), 0] and np.isnan(gap.corr_coeff).all() and not gap.tested.any()
    assert np.isnan(gap.p_value).all() and np.isnan(gap.p_corrected).all() and gap.sums_q[1] == 0
    const = compare.mantel_correlogram(x, np.full(len(x), 2.5), n_classes=3, cutoff=False, permutations=9, seed=1, keep_stats=True, device=None)
    assert np.isnan(const.corr_coeff).all() and not const.tested.any() and np.isnan(const.perm_stats).all()
    assert const.n_ge.tolist() == [9, 9, 9] and const.n_le.tolist() == [9, 9, 9]      # (every relabelling ties)


def test_more_classes_than_the_limit():
    x, y = _points(20, 6)
    assert _capi.CLASS_MAX == 64 and len(compare.mantel_correlogram(x, y, n_classes=64, permutations=1, seed=1, device=None)) == 64
    with pytest.raises(ValueError, match="65 classes: at most 64"):
        compare.mantel_correlogram(x, y, n_classes=65, device=None)
    with pytest.raises(ValueError, match="65 classes: at most 64"):
        compare.mantel_correlogram(x, y, breaks=np.linspace(0.0, 1.0, 66), device=None)
    for kw in ({"method": "kendall"}, {"correction": "fdr"}, {"permutations": -1}, {"seed": -1}, {"stream": -1}, {"chunk_tasks": -1}, {"n_classes": 0}):
        with pytest.raises(ValueError):
            compare.mantel_correlogram(x, y, device=None, **kw)
    with pytest.raises(ValueError, match="y has 5 objects, x has 20"):
        compare.mantel_correlogram(x, np.arange(10.0), device=None)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_class_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_class")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_class.cpp"), os.path.join(csrc, "class_plan.cpp"),
                           os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize class ok" in out.stdout
