"""The compare path without a GPU: its C ABI (exports, version, argument errors), the statistics of DistanceComparison
and its merge, the name -> id resolution of SuchTree.compare_distances, and the reduction kernel's registers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_path
from suchtree_amd import NodeNotFoundError, SuchTree, _capi, build as st_build
from suchtree_amd.compare import DistanceComparison, _needs_data_range, histogram_edges


@pytest.fixture(scope="module")
def lib():
    st_build.build()
    return _capi.load()


def test_compare_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    for name in ("st_compare_triangle_host", "st_compare_pairs_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS
        assert getattr(lib, name) is not None
    assert "typedef struct st_pair_moments" in header
    assert lib.st_api_version() == 7 == _capi.API_VERSION
    assert ctypes.sizeof(_capi.PairMoments) == 8 + 11 * 8


def _edges(n, lo=0.0, hi=1.0):
    return np.linspace(lo, hi, n + 1)


def test_compare_argument_errors_without_a_gpu(lib):
    out = _capi.PairMoments()
    bad = ctypes.c_int64(0)
    ids = np.arange(4, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def tri(ex, bx, ey, by, hist, tx=None, ty=None):
        return lib.st_compare_triangle_host(tx, ty, p(ids), p(ids), 4, 0, 6, p(ex), bx, p(ey), by, ctypes.byref(out), p(hist),
                                            ctypes.byref(bad))

    def prs(ex, bx, ey, by, hist):
        pairs = np.zeros((3, 2), dtype=np.int64)
        return lib.st_compare_pairs_host(None, None, p(pairs), p(pairs), 3, p(ex), bx, p(ey), by, ctypes.byref(out), p(hist),
                                         ctypes.byref(bad))

    # NULL trees
    for fn in (tri, prs):
        assert fn(None, 0, None, 0, None) == _capi.ST_ERR_ARG
        assert "NULL" in _capi.last_error()
    # too many cells (129 x 128 > 16384); 128 x 128 passes the histogram checks and stops at the NULL trees
    h = np.zeros(129 * 128, dtype=np.int64)
    for fn in (tri, prs):
        assert fn(_edges(129), 129, _edges(128), 128, h) == _capi.ST_ERR_ARG
        assert "cells" in _capi.last_error()
        assert fn(_edges(128), 128, _edges(128), 128, h) == _capi.ST_ERR_ARG
        assert "tree" in _capi.last_error()
    # edges not increasing, not finite, empty range, bins < 1
    dec = _edges(8)[::-1].copy()
    nan = _edges(8)
    nan[3] = np.nan
    flat = np.zeros(9)
    for ex in (dec, nan, flat):
        assert tri(ex, 8, _edges(8), 8, np.zeros(64, dtype=np.int64)) == _capi.ST_ERR_ARG
        assert "edge" in _capi.last_error()
        assert prs(_edges(8), 8, ex, 8, np.zeros(64, dtype=np.int64)) == _capi.ST_ERR_ARG
        assert "edge" in _capi.last_error()
    assert tri(_edges(8), 0, _edges(8), 8, np.zeros(64, dtype=np.int64)) == _capi.ST_ERR_ARG
    assert "bins" in _capi.last_error()
    # one of edges / out_hist NULL and the others not
    for args in ((None, 8, _edges(8), 8, np.zeros(64, dtype=np.int64)), (_edges(8), 8, None, 8, np.zeros(64, dtype=np.int64)),
                 (_edges(8), 8, _edges(8), 8, None)):
        for fn in (tri, prs):
            assert fn(*args) == _capi.ST_ERR_ARG
            assert "all be given or all be NULL" in _capi.last_error()


def _stats_from_data(x, y, shift=(0.0, 0.0), **kw):
    cx, cy = shift
    dx, dy = x - cx, y - cy
    return DistanceComparison.from_sums(len(x), cx, cy, dx.sum(), dy.sum(), (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum(),
                                        x.min(), x.max(), y.min(), y.max(), **kw)


def test_distance_comparison_against_numpy():
    rng = np.random.default_rng(5)
    x = rng.gamma(4.0, 0.3, 200_001) + 50.0          # a large offset: the shift is what keeps the sums exact enough
    y = 0.7 * x + rng.normal(0, 0.2, len(x))
    shift = (float(x[:4096].mean()), float(y[:4096].mean()))
    c = _stats_from_data(x, y, shift)
    assert c.n_pairs == len(x) and c.n_leaves is None
    for got, want in ((c.mean_x, x.mean()), (c.mean_y, y.mean()), (c.var_x, np.var(x)), (c.var_y, np.var(y)),
                      (c.cov, np.cov(x, y, bias=True)[0, 1])):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-12
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max())
    # merge of two halves (different shifts, as two calls would have) equals the whole
    h = 123_457
    a = _stats_from_data(x[:h], y[:h], (float(x[:4096].mean()), float(y[:4096].mean())))
    b = _stats_from_data(x[h:], y[h:], (float(x[h:h + 4096].mean()), float(y[h:h + 4096].mean())))
    m = DistanceComparison.merge(a, b)
    assert m.n_pairs == c.n_pairs
    for k in ("mean_x", "mean_y", "var_x", "var_y", "cov", "pearson_r"):
        assert abs(getattr(m, k) - getattr(c, k)) <= 1e-12 * max(1.0, abs(getattr(c, k))), k
    assert (m.min_x, m.max_x, m.min_y, m.max_y) == (c.min_x, c.max_x, c.min_y, c.max_y)
    assert DistanceComparison.merge(a, DistanceComparison.from_sums(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)) is a


def test_distance_comparison_degenerate_cases():
    e = DistanceComparison.from_sums(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, np.nan, np.nan, np.nan, np.nan)
    assert e.n_pairs == 0 and np.isnan(e.mean_x) and np.isnan(e.pearson_r) and np.isnan(e.var_y)
    x = np.full(10, 2.5)
    y = np.arange(10.0)
    c = _stats_from_data(x, y)
    assert c.var_x == 0.0 and np.isnan(c.pearson_r) and c.var_y == np.var(y)


def test_merged_histograms_add_and_must_share_edges():
    rng = np.random.default_rng(1)
    x, y = rng.random(1000), rng.random(1000)
    ex, ey = _edges(4), _edges(5)
    H = lambda a, b: np.histogram2d(a, b, bins=(ex, ey))[0].astype(np.int64)  # noqa: E731
    a = _stats_from_data(x[:400], y[:400], hist=H(x[:400], y[:400]), xedges=ex, yedges=ey)
    b = _stats_from_data(x[400:], y[400:], hist=H(x[400:], y[400:]), xedges=ex, yedges=ey)
    assert np.array_equal(DistanceComparison.merge(a, b).hist, H(x, y))
    other = _stats_from_data(x[400:], y[400:], hist=np.zeros((4, 4), np.int64), xedges=_edges(4), yedges=_edges(4))
    with pytest.raises(ValueError):
        DistanceComparison.merge(a, other)


def test_merge_keeps_infinite_squares_infinite():
    """b holds an infinite x: its squares are +inf about any shift, also moved to a's larger shift (inf - inf before)."""
    a = DistanceComparison.from_sums(3, 5.0, 1.0, 0.5, 0.25, 2.0, 1.0, 0.5, 4.0, 6.0, 0.5, 1.5)
    b = DistanceComparison.from_sums(2, 0.0, 1.0, np.inf, 0.5, np.inf, 0.5, np.inf, 1.0, np.inf, 1.0, 1.5)
    m = DistanceComparison.merge(a, b)
    assert m.n_pairs == 5 and m.sx == np.inf and m.sxx == np.inf and m.max_x == np.inf
    assert (m.sy, m.syy) == (0.75, 1.5)
    c = DistanceComparison.from_sums(2, 1.0, 1.0, np.nan, 0.5, np.nan, 0.5, np.nan, 1.0, 2.0, 1.0, 1.5)
    assert np.isnan(DistanceComparison.merge(a, c).sxx)


def test_histogram_edges_are_numpy_s():
    rng = np.random.default_rng(2)
    x, y = rng.random(500) * 3, rng.random(500) + 7
    for bins, rng_ in ((64, None), ((8, 16), None), (10, [(0.5, 2.0), (7.2, 7.9)]), ((_edges(3), _edges(5, 7, 8)), None)):
        _, wx, wy = np.histogram2d(x, y, bins=bins, range=rng_)
        gx, gy = histogram_edges(bins, rng_, (x.min(), x.max(), y.min(), y.max()))
        assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    # an empty range widens by 0.5 as numpy's does
    _, wx, wy = np.histogram2d(np.full(5, 3.0), np.arange(5.0), bins=4)
    gx, gy = histogram_edges(4, None, (3.0, 3.0, 0.0, 4.0))
    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert _needs_data_range(64, None) and _needs_data_range((4, _edges(3)), None)
    assert not _needs_data_range(64, [(0, 1), (0, 1)]) and not _needs_data_range((_edges(3), _edges(4)), None)


def _named(parent, dist, names):
    return SuchTree((parent, dist, names))


def test_shared_leaf_resolution_and_unknown_names():
    from suchtree_amd import synth
    p, d = synth.balanced_tree(4)                               # 16 leaves
    a = _named(p, d, ["t%d" % i for i in range(16)])
    names_b = ["t%d" % i for i in (15, 3, 99, 7, 0, 12, 98, 5, 4, 1, 2, 97, 6, 8, 9, 96)]
    b = _named(p, d, names_b)
    names, ids_a, ids_b = a.shared_leaves(b)
    assert names == [n for n in sorted(a.leaves, key=a.leaves.get) if n in b.leaves]
    assert set(names) == set(a.leaves) & set(b.leaves) and len(names) == 12
    assert list(ids_a) == sorted(ids_a) == [a.leaves[n] for n in names]
    assert list(ids_b) == [b.leaves[n] for n in names]
    # unknown names raise before anything touches a GPU, as in distances_by_name
    with pytest.raises(NodeNotFoundError):
        a.compare_distances(b, leaves=["t1", "t10"])               # t10 is not in b
    with pytest.raises(NodeNotFoundError):
        a.compare_distances(b, pairs=[("t1", "t2"), ("t3", "nope")])
    with pytest.raises(TypeError):
        a.compare_distances(b, pairs=[("t1", 2)])
    with pytest.raises(ValueError):
        a.compare_distances(b, leaves=["t1"], pairs=[("t1", "t2")])


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_compare_kernels_compile_for_gfx950_without_spills(tmp_path):
    unit = tmp_path / "compare_unit.hip"
    unit.write_text('#include <hip/hip_runtime.h>\n#include "device_common.h"\n#include "kernels_compare.h"\n'
                    "template __global__ void st::k_pair_moments<true>(const float *, const float *, long long, const double *, int,"
                    " st::CmpPartial *, st::CmpHist);\n"
                    "template __global__ void st::k_pair_moments<false>(const float *, const float *, long long, const double *, int,"
                    " st::CmpPartial *, st::CmpHist);\n")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "suchtree_amd", "csrc"), "--cuda-device-only",
                          "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "unit.o"), str(unit)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\bVGPRs: (\d+)", line)
        if m and name:
            res.setdefault(name, {})["vgpr"] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            res.setdefault(name, {})["spill"] = int(m.group(1))
    kernels = {k: v for k, v in res.items() if "k_pair" in k}
    assert len(kernels) >= 4, res                                  # both forms, the shift and the final pass
    for k, v in kernels.items():
        assert v["spill"] == 0 and v["vgpr"] <= 128, (k, v)       # 256-lane workgroups, several per CU
