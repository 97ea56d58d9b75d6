"""Exact Kendall tau-b counts without a GPU: st_kendall_host (the key, the tie rule and the counts the GPU path shares,
suchtree_amd/csrc/kendall_plan.cpp) against an O(n^2) count in numpy -- equal, not close -- and scipy's tau; the tiled
restatement that walks tiles and merge levels as the kernels do; the ABI; the Python fields; the new kernels' resources;
the new host code under ASan / UBSan."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.stats import kendalltau

from conftest import ROOT
from kendall_reference import brute_counts, heavy_columns, tau_b, tie_sum
from rank_reference import host_columns
from suchtree_amd import _capi
from suchtree_amd.compare import DistanceComparison, kendall_fields, kendall_from_counts

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "suchtree_amd", "csrc")
NAMES = ("kendall_tau", "concordant", "discordant", "ties_x", "ties_y", "ties_xy")


def _tau(c):
    return kendall_fields(c)["kendall_tau"]


def _equal(c, ref):
    assert c.as_tuple() == tuple(ref), (c.as_tuple(), tuple(ref))


@pytest.mark.parametrize("case", list(host_columns()))
def test_counts_equal_the_quadratic_count(case):
    x, y = (v[:2000] for v in host_columns()[case])
    c = _capi.kendall_host(x, y)
    ref = brute_counts(x, y)
    _equal(c, ref)
    assert (c.ties_x, c.ties_y) == (tie_sum(x), tie_sum(y))
    n0 = len(x) * (len(x) - 1) // 2
    assert c.concordant + c.discordant + c.ties_x + c.ties_y - c.ties_xy == n0
    got, want = _tau(c), kendalltau(x, y)[0]
    print("%s: tau %.17g, scipy %.17g, from the reference counts %.17g" % (case, got, want, tau_b(ref)))
    assert abs(got - want) < 1e-12 and abs(got - tau_b(ref)) < 1e-15


@pytest.mark.parametrize("case", list(host_columns()))
def test_tau_agrees_with_scipy_on_the_full_columns(case):
    x, y = host_columns()[case]
    c = _capi.kendall_host(x, y)
    got, want = _tau(c), kendalltau(x, y)[0]
    print("%s: n %d, tau %.17g, scipy %.17g, difference %.3g" % (case, len(x), got, want, got - want))
    assert abs(got - want) < 1e-12
    assert (c.ties_x, c.ties_y) == (tie_sum(x), tie_sum(y))


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_heavy_ties(seed):
    x, y = heavy_columns(1500, seed)
    _equal(_capi.kendall_host(x, y), brute_counts(x, y))


def test_small_constant_identical_and_negated_columns():
    for n in (0, 1, 2):
        x, y = np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32)[::-1].copy()
        c = _capi.kendall_host(x, y)
        _equal(c, brute_counts(x, y))
        assert math.isnan(_tau(c)) if n < 2 else _tau(c) == -1.0
    rng = np.random.default_rng(44)
    v = (rng.integers(-30, 30, 900) * 0.5).astype(np.float32)
    const = np.full(900, 2.5, np.float32)
    n0 = 900 * 899 // 2
    for x, y in ((const, v), (v, const), (const, const)):
        c = _capi.kendall_host(x, y)
        _equal(c, brute_counts(x, y))
        assert math.isnan(_tau(c)) and math.isnan(kendalltau(x, y)[0])
        assert c.ties_x == (n0 if x is const else tie_sum(v)) and c.ties_y == (n0 if y is const else tie_sum(v))
    same = _capi.kendall_host(v, v)
    _equal(same, brute_counts(v, v))
    assert same.discordant == 0 and same.ties_x == same.ties_y == same.ties_xy and _tau(same) == 1.0
    neg = _capi.kendall_host(v, -v)
    _equal(neg, brute_counts(v, -v))
    assert neg.concordant == 0 and neg.discordant == n0 - neg.ties_x and _tau(neg) == -1.0


def test_zeros_infinities_and_nan():
    x = np.float32([0.0, -0.0, np.inf, -np.inf, 1.0, -0.0, np.inf, 3.0e-45])
    y = np.float32([-0.0, 0.0, -np.inf, np.inf, -0.0, 2.0, np.inf, -np.inf])
    c = _capi.kendall_host(x, y)
    _equal(c, brute_counts(x, y))
    assert c.ties_x == 3 + 1 and c.ties_y == 3 + 1 + 1 and c.ties_xy == 1      # the zeros tie whatever their sign
    assert abs(_tau(c) - kendalltau(x, y)[0]) < 1e-12
    for bad_x, bad_y, n_nan in ((1, None, 1), (None, 2, 1), (1, 1, 1), (1, 2, 2)):
        xs, ys = x.copy(), y.copy()
        if bad_x is not None:
            xs[bad_x] = np.nan
        if bad_y is not None:
            ys[bad_y] = np.nan
        c = _capi.kendall_host(xs, ys)
        assert c.as_tuple() == (8, n_nan, 0, 0, 0, 0) and c.concordant == 0
        assert math.isnan(_tau(c)) and math.isnan(kendalltau(xs, ys)[0])
        _equal(c, brute_counts(xs, ys))


def test_reversed_column_passes_two_to_the_32():
    n = 200_000
    x = np.arange(n, dtype=np.float32)
    c = _capi.kendall_host(x, x[::-1].copy())
    assert c.as_tuple() == (n, 0, 19_999_900_000, 0, 0, 0) and c.discordant > 2 ** 32 and _tau(c) == -1.0


@pytest.fixture(scope="module")
def tiled(tmp_path_factory):
    """kendall_host_tiled behind a C function (tests/emu/kendall_tiled.cpp), built with plain g++."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = str(tmp_path_factory.mktemp("kendall") / "libkendall_tiled.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", lib, os.path.join(ROOT, "tests", "emu", "kendall_tiled.cpp"),
                           os.path.join(CSRC, "kendall_plan.cpp"), os.path.join(CSRC, "rank_plan.cpp")])
    L = ctypes.CDLL(lib)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.kendall_tiled.argtypes = [vp, vp, i64, i64, ctypes.POINTER(_capi.KendallCounts)]
    L.kendall_plain.argtypes = [vp, vp, i64, ctypes.POINTER(_capi.KendallCounts)]

    def run(x, y, tile):
        out = _capi.KendallCounts()
        p = lambda a: a.ctypes.data_as(vp) if len(a) else None  # noqa: E731
        assert L.kendall_tiled(p(x), p(y), len(x), tile, ctypes.byref(out)) == 0
        return out
    return run


@pytest.mark.parametrize("tile", [4, 8, 64])
def test_tiled_restatement_equals_the_host_at_every_small_size(tiled, tile):
    """Every n from 0 to 4 tile + 1: a single tile, a lone left run, a short right run, full levels."""
    for n in range(0, 4 * tile + 2):
        for x, y in (heavy_columns(n, 50 + n), (np.random.default_rng(n).random(n).astype(np.float32),
                                                 np.random.default_rng(n + 1).random(n).astype(np.float32))):
            want = _capi.kendall_host(x, y)
            assert tiled(x, y, tile).as_tuple() == want.as_tuple(), (n, tile)
            if n <= 40:
                _equal(want, brute_counts(x, y))


@pytest.mark.parametrize("tile", [4, 8, 64])
@pytest.mark.parametrize("n", [9_973, 10_000, 10_241])
def test_tiled_restatement_equals_the_host_around_ten_thousand(tiled, tile, n):
    rng = np.random.default_rng(n)
    x = (rng.integers(0, 300, n) * 0.25).astype(np.float32)
    y = (x * rng.integers(0, 2, n) + rng.integers(0, 50, n)).astype(np.float32)
    assert tiled(x, y, tile).as_tuple() == _capi.kendall_host(x, y).as_tuple()


def test_abi_is_additive():
    lib = _capi.load()
    for name in ("st_compare_triangle_kendall_host", "st_compare_pairs_kendall_host", "st_kendall_arrays_host", "st_kendall_host"):
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
    assert lib.st_api_version() == 7 == _capi.API_VERSION
    assert ctypes.sizeof(_capi.KendallCounts) == 48
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    assert re.search(r"typedef struct st_kendall_counts \{", header) and "#define ST_API_VERSION 7" in header
    assert int(re.search(r"#define ST_KENDALL_TILE (\d+)", header).group(1)) == _capi.KENDALL_TILE
    out, counts, bad = _capi.PairMoments(), _capi.KendallCounts(), ctypes.c_int64(0)
    assert lib.st_compare_triangle_kendall_host(None, None, None, None, 0, 0, 0, 0, ctypes.byref(out), ctypes.byref(counts),
                                                ctypes.byref(bad)) == _capi.ST_ERR_ARG and "NULL" in _capi.last_error()
    assert lib.st_compare_triangle_kendall_host(None, None, None, None, 0, 0, 0, 0, ctypes.byref(out), None, ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert lib.st_compare_pairs_kendall_host(None, None, None, None, 0, 0, None, ctypes.byref(counts), ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert lib.st_compare_pairs_kendall_host(None, None, None, None, 0, 0, ctypes.byref(out), ctypes.byref(counts), ctypes.byref(bad)) == _capi.ST_ERR_ARG
    one = np.zeros(1, np.float32).ctypes.data_as(ctypes.c_void_p)
    for call in (lambda *a: lib.st_kendall_host(*a), lambda *a: lib.st_kendall_arrays_host(0, *a)):
        assert call(None, None, 1, ctypes.byref(counts)) == _capi.ST_ERR_ARG and "NULL" in _capi.last_error()
        assert call(one, one, 1, None) == _capi.ST_ERR_ARG
        assert call(one, one, -1, ctypes.byref(counts)) == _capi.ST_ERR_ARG
        assert call(None, None, 2 ** 31, ctypes.byref(counts)) == _capi.ST_ERR_ARG and "2147483647" in _capi.last_error()
    assert lib.st_kendall_arrays_host(0, None, None, 0, ctypes.byref(counts)) == _capi.ST_OK and counts.as_tuple() == (0,) * 6
    with pytest.raises(ValueError):
        _capi.kendall_host(np.zeros(3, np.float32), np.zeros(4, np.float32))


def test_distance_comparison_kendall_fields_default_to_none_and_merge_drops_them():
    rng = np.random.default_rng(45)
    x, y = rng.integers(0, 40, 500).astype(np.float32), rng.integers(0, 40, 500).astype(np.float32)

    def comparison(x, y, kendall):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return DistanceComparison.from_sums(len(x), 0.0, 0.0, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(),
                                            x.min(), x.max(), y.min(), y.max(), kendall=kendall)
    plain = comparison(x, y, None)
    assert all(getattr(plain, k) is None for k in NAMES)
    a, b = comparison(x[:300], y[:300], _capi.kendall_host(x[:300], y[:300])), comparison(x[300:], y[300:], _capi.kendall_host(x[300:], y[300:]))
    assert all(isinstance(getattr(a, k), int) for k in NAMES[1:]) and a.spearman_r is None
    ref = brute_counts(x[:300], y[:300])
    assert (a.discordant, a.ties_x, a.ties_y, a.ties_xy) == tuple(ref)[2:]
    assert a.concordant == 300 * 299 // 2 - ref.ties_x - ref.ties_y + ref.ties_xy - ref.discordant
    assert abs(a.kendall_tau - kendalltau(x[:300], y[:300])[0]) < 1e-12
    merged = DistanceComparison.merge(a, b)
    assert merged.n_pairs == 500 and all(getattr(merged, k) is None for k in NAMES)
    empty = DistanceComparison.from_sums(0, 0, 0, 0, 0, 0, 0, 0, np.nan, np.nan, np.nan, np.nan)
    for m in (DistanceComparison.merge(a, empty), DistanceComparison.merge(empty, a)):
        assert m.n_pairs == 300 and all(getattr(m, k) is None for k in NAMES)


def test_kendall_tau_is_exactly_one_when_the_counts_say_so():
    """Identical columns: concordant == n0 - ties_x == n0 - ties_y.  One root of the product, so 1.0 and -1.0 exactly."""
    rng = np.random.default_rng(46)
    for _ in range(3000):
        n = int(rng.integers(2, 2 ** 31))
        n0 = n * (n - 1) // 2
        ties = int(rng.integers(0, n0))      # (n0 - ties >= 1: magnitudes up to 2^61)
        assert kendall_from_counts(n, 0, n0 - ties, 0, ties, ties) == 1.0
        assert kendall_from_counts(n, 0, 0, n0 - ties, ties, ties) == -1.0
    n = 2 ** 31 - 1
    assert kendall_from_counts(n, 0, n * (n - 1) // 2, 0, 0, 0) == 1.0 and n * (n - 1) // 2 > 2 ** 60
    assert math.isnan(kendall_from_counts(n, 1, 0, 0, 0, 0)) and math.isnan(kendall_from_counts(1, 0, 0, 0, 0, 0))
    assert math.isnan(kendall_from_counts(4, 0, 0, 0, 6, 0)) and math.isnan(kendall_from_counts(4, 0, 0, 0, 0, 6))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kendall_kernels_use_no_scratch_and_bounded_lds(tmp_path):
    """256-lane workgroups: no spills, no scratch -- a lane's eight keys, sorted by fixed indices, stay in registers -- and
    at most the 32 KiB of two tiles of 64-bit keys plus a few words of LDS.  LDS then admits five
    workgroups per CU, five waves per SIMD; 512 / 5 = 102 registers per lane keep that many resident, so at most 96."""
    unit = tmp_path / "kendall_unit.hip"
    unit.write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "kernels_kendall.h"\n'
                    "namespace st {\n"
                    "template __global__ void k_kendall_tile_sort<unsigned long long, false>(const unsigned long long *, unsigned long long *, long long, unsigned long long *);\n"
                    "template __global__ void k_kendall_tile_sort<uint32_t, true>(const uint32_t *, uint32_t *, long long, unsigned long long *);\n"
                    "template __global__ void k_kendall_merge<unsigned long long, false>(const unsigned long long *, unsigned long long *, long long, long long, unsigned long long *);\n"
                    "template __global__ void k_kendall_merge<uint32_t, true>(const uint32_t *, uint32_t *, long long, long long, unsigned long long *);\n"
                    "template __global__ void k_kendall_tie_blocks<unsigned long long>(const unsigned long long *, long long, int, int *);\n"
                    "template __global__ void k_kendall_tie_blocks<uint32_t>(const uint32_t *, long long, int, int *);\n"
                    "template __global__ void k_kendall_tie_sums<unsigned long long>(const unsigned long long *, long long, int, const int *, unsigned long long *);\n"
                    "template __global__ void k_kendall_tie_sums<uint32_t>(const uint32_t *, long long, int, const int *, unsigned long long *);\n"
                    "}\n")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "-I", CSRC, "--cuda-device-only",
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
    kernels = {k: v for k, v in res.items() if "k_kendall_" in k}
    print(kernels)
    for frag in ("k_kendall_keys", "k_kendall_tile_sortIyLb0", "k_kendall_tile_sortIjLb1", "k_kendall_mergeIyLb0", "k_kendall_mergeIjLb1",
                 "k_kendall_low_words", "k_kendall_tie_blocksIy", "k_kendall_tie_blocksIj", "k_kendall_tie_carry", "k_kendall_tie_sumsIy",
                 "k_kendall_tie_sumsIj", "k_kendall_final"):
        assert any(frag in k for k in kernels), frag
    for k, v in kernels.items():
        assert v["scratch"] == 0 and v["spill"] == 0 and v["sspill"] == 0, (k, v)
        assert v["vgpr"] <= 96 and v["sgpr"] <= 96, (k, v)
        assert v["lds"] <= 2 * _capi.KENDALL_TILE * 8 + 64, (k, v)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_kendall_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_kendall")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_kendall.cpp"), os.path.join(CSRC, "kendall_plan.cpp"),
                           os.path.join(CSRC, "rank_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize kendall ok" in out.stdout
