"""Exact Spearman rank sums without a GPU: st_spearman_host (the key transform, midranks and tie arithmetic the GPU path
shares, suchtree_amd/csrc/rank_plan.cpp) against Python big-int sums built from scipy.stats.rankdata -- equal, not
close; the Python fields; the new kernels' resources; the new host code under ASan / UBSan."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.stats import spearmanr

from conftest import ROOT
from rank_reference import host_columns as _columns, perfect_tree_sums, scipy_midrank_sums as _want, tie_identity as _tie_identity
from suchtree_amd import _capi
from suchtree_amd.compare import DistanceComparison, rank_fields, spearman_from_sums

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("case", list(_columns()))
def test_sums_equal_scipy_midranks(case):
    x, y = _columns()[case]
    r = _capi.spearman_host(x, y)
    sxy, sxx, syy = _want(x, y)
    assert (r.n, r.n_nan) == (len(x), 0)
    assert (r.sxy, r.sxx, r.syy) == (sxy, sxx, syy)
    assert (r.distinct_x, r.distinct_y) == (len(np.unique(x)), len(np.unique(y)))
    assert r.sxx == _tie_identity(x) and r.syy == _tie_identity(y)
    got, want = spearman_from_sums(r.n, r.n_nan, r.sxy, r.sxx, r.syy), spearmanr(x, y)[0]
    print("%s: spearman_r %.17g, scipy %.17g, difference %.3g" % (case, got, want, got - want))
    assert abs(got - want) < 1e-12


def test_identical_and_negated_columns():
    rng = np.random.default_rng(32)
    x = (rng.integers(-500, 500, 150_000) * 0.5).astype(np.float32)
    x[::1000] = np.inf
    r = _capi.spearman_host(x, x)
    assert r.sxy == r.sxx == r.syy == _tie_identity(x) and rank_fields(r)["spearman_r"] == 1.0
    m = _capi.spearman_host(x, -x)
    assert m.sxy == -m.sxx and m.sxx == m.syy == r.sxx and rank_fields(m)["spearman_r"] == -1.0
    # -0.0 ties with +0.0 on either side
    z = _capi.spearman_host(np.float32([0.0, -0.0, 1.0, -1.0]), np.float32([-0.0, 0.0, 2.0, -2.0]))
    assert z.distinct_x == z.distinct_y == 3 and z.sxy == z.sxx == z.syy == (4 ** 3 - 4 - 6) // 3


def test_spearman_r_is_exactly_one_when_the_sums_are_equal():
    """sqrt(s) * sqrt(s) misses s by an ulp for some s (the triangle of a perfect tree of 1024 leaves against itself gave
    0.9999999999999998): spearman_from_sums takes one root of the product."""
    for L in range(2, 17):
        s = perfect_tree_sums(L, "identity")
        assert s.sxy == s.sxx == s.syy
        assert spearman_from_sums(s.n, 0, s.sxy, s.sxx, s.syy) == 1.0 and spearman_from_sums(s.n, 0, -s.sxy, s.sxx, s.syy) == -1.0
    rng = np.random.default_rng(34)
    for s in rng.integers(1, 2 ** 62, 2000):
        s = int(s) * int(rng.integers(1, 2 ** 31))
        assert spearman_from_sums(5, 0, s, s, s) == 1.0 and spearman_from_sums(5, 0, -s, s, s) == -1.0


def test_nan_empty_single_and_constant_columns_give_nan():
    x = np.float32([1, 2, np.nan, 4, 5])
    y = np.float32([np.nan, 1, np.nan, 3, 2])
    r = _capi.spearman_host(x, y)
    assert (r.n, r.n_nan) == (5, 2) and (r.sxy, r.sxx, r.syy, r.distinct_x, r.distinct_y) == (0, 0, 0, 0, 0)
    assert math.isnan(rank_fields(r)["spearman_r"]) and math.isnan(spearmanr(x, y)[0])
    for n in (0, 1):
        e = _capi.spearman_host(np.zeros(n, np.float32), np.zeros(n, np.float32))
        assert (e.n, e.sxy, e.sxx, e.syy) == (n, 0, 0, 0) and math.isnan(rank_fields(e)["spearman_r"])
    c = _capi.spearman_host(np.float32([3, 3, 3, 3]), np.float32([1, 2, 3, 4]))
    assert c.sxx == 0 and c.syy == 20 and c.distinct_x == 1 and math.isnan(rank_fields(c)["spearman_r"])
    with pytest.raises(ValueError):
        _capi.spearman_host(np.zeros(3, np.float32), np.zeros(4, np.float32))


def test_abi_is_additive():
    lib = _capi.load()
    for name in ("st_compare_triangle_ranks_host", "st_compare_pairs_ranks_host", "st_spearman_host"):
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
    assert lib.st_api_version() == 7 == _capi.API_VERSION
    assert ctypes.sizeof(_capi.RankSums) == 80
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    assert re.search(r"typedef struct st_rank_sums \{", header) and "#define ST_API_VERSION 7" in header
    # argument errors of the GPU entry points that need no GPU
    out, ranks, bad = _capi.PairMoments(), _capi.RankSums(), ctypes.c_int64(0)
    assert lib.st_compare_triangle_ranks_host(None, None, None, None, 0, 0, 0, 0, ctypes.byref(out), ctypes.byref(ranks),
                                              ctypes.byref(bad)) == _capi.ST_ERR_ARG and "NULL" in _capi.last_error()
    assert lib.st_compare_pairs_ranks_host(None, None, None, None, 0, 0, None, ctypes.byref(ranks), ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert lib.st_spearman_host(None, None, 2**31, ctypes.byref(ranks)) == _capi.ST_ERR_ARG and "2147483647" in _capi.last_error()


def test_distance_comparison_rank_fields_default_to_none_and_merge_drops_them():
    rng = np.random.default_rng(33)
    x, y = rng.random(500).astype(np.float32), rng.random(500).astype(np.float32)

    def comparison(x, y, ranks):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return DistanceComparison.from_sums(len(x), 0.0, 0.0, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(),
                                            x.min(), x.max(), y.min(), y.max(), ranks=ranks)
    names = ("spearman_r", "rank_sxy", "rank_sxx", "rank_syy", "distinct_x", "distinct_y")
    plain = comparison(x, y, None)
    assert all(getattr(plain, k) is None for k in names)
    a, b = comparison(x[:300], y[:300], _capi.spearman_host(x[:300], y[:300])), comparison(x[300:], y[300:], _capi.spearman_host(x[300:], y[300:]))
    assert isinstance(a.rank_sxy, int) and isinstance(a.rank_sxx, int) and a.distinct_x == len(np.unique(x[:300]))
    assert abs(a.spearman_r - spearmanr(x[:300], y[:300])[0]) < 1e-12
    merged = DistanceComparison.merge(a, b)
    assert merged.n_pairs == 500 and all(getattr(merged, k) is None for k in names)
    assert abs(merged.pearson_r - np.corrcoef(x.astype(np.float64), y.astype(np.float64))[0, 1]) < 1e-12
    empty = DistanceComparison.from_sums(0, 0, 0, 0, 0, 0, 0, 0, np.nan, np.nan, np.nan, np.nan)
    for m in (DistanceComparison.merge(a, empty), DistanceComparison.merge(empty, a)):
        assert m.n_pairs == 300 and all(getattr(m, k) is None for k in names)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_rank_kernels_use_no_scratch_and_few_registers(tmp_path):
    """256-lane workgroups, several per CU: at most 64 VGPRs (8 waves per SIMD), no spills, no scratch -- the 128-bit
    accumulators and their shuffles stay in registers."""
    unit = tmp_path / "ranks_unit.hip"
    unit.write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "kernels_ranks.h"\n')
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
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
                         ("sspill", r"SGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    kernels = {k: v for k, v in res.items() if "k_rank_" in k}
    print(kernels)
    for frag in ("k_rank_occupancy", "k_rank_count", "k_rank_block_sums", "k_rank_scan_blocks", "k_rank_scan_apply", "k_rank_dotE", "k_rank_dot_final"):
        assert any(frag in k for k in kernels), frag
    for k, v in kernels.items():
        assert v["scratch"] == 0 and v["spill"] == 0 and v["sspill"] == 0, (k, v)
        assert v["vgpr"] <= 64 and v["sgpr"] <= 96, (k, v)
        assert v["lds"] <= 40 * 1024, (k, v)          # two 4096-entry slot maps or histograms: four workgroups per CU


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rank_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_ranks")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_ranks.cpp"),
                           os.path.join(ROOT, "suchtree_amd", "csrc", "rank_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize ranks ok" in out.stdout
