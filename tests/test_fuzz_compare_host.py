"""Seeded sessions of tests/fuzz_compare.py on the host layer (no GPU): the references that the device sessions take as
their yardstick against independent definitions, on the CPU oracle's distances of drawn trees and pairs at small sizes --
compare_reference._Sums against np.mean, np.var, np.cov, np.corrcoef and the contract's searchsorted histogram rule,
rank_reference.rank_sums against scipy's midranks and st_spearman_host, kendall_reference.brute_counts against
st_kendall_host and scipy.stats.kendalltau, the pick rule of the quartet classes against the four-point rule and the oracle's
sister pairs, the restated clade layout against st_clade_plan, the Hommola permutation against st_hommola_permutation -- and
the linked family, SuchLinkedTrees' link list, _links_in_order and _partner_rows against the dense matrix.  The census of the device sessions is asserted here from the draws alone, so a
hollowed generator fails before a GPU sees it."""
import pytest

import fuzz_compare
from suchtree_amd import build as st_build

CASES = 300
SEEDS = {"moments": (1, 2), "ranks": (1, 2), "kendall2": (3, 5), "rows": (1, 2), "quartets": (1, 2), "clades": (1, 2), "hommola": (1, 2), "linked": (1, 2)}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()


@pytest.mark.parametrize("family,seed", [(f, s) for f in fuzz_compare.FAMILIES for s in SEEDS[f]])
def test_references_against_independent_definitions(family, seed):
    reached = fuzz_compare.run(family, seed, CASES, "host")
    print("%s seed %d: %d cases; %s" % (family, seed, CASES, dict(sorted(reached.items()))))


@pytest.mark.parametrize("family", [f for f in fuzz_compare.FAMILIES if f in fuzz_compare.REQUIRED["device"]])
def test_census_of_the_device_sessions_holds(family):
    import test_gpu_fuzz_compare as gpu
    for seed in gpu.SEEDS[family]:
        reached = fuzz_compare.census(family, seed, gpu.CASES, "device")
        print("%s seed %d: %s" % (family, seed, dict(sorted(reached.items()))))
        assert fuzz_compare.missing(family, reached, "device") == [], seed


def _nearly_constant():
    """float32 columns as a clade's would be: a first pair far from the rest, the rest within a few 1e-5 of one value"""
    import numpy as np
    rng = np.random.default_rng(5)
    x = (10.45 + 2e-5 * rng.standard_normal(4000)).astype(np.float32).astype(np.float64)
    y = (3.0 + rng.random(4000)).astype(np.float32).astype(np.float64)
    x[0] = 10.0
    return x, y


def _record(x, y, shift_x, shift_y):
    from suchtree_amd.compare import DistanceComparison
    dx, dy = x - shift_x, y - shift_y
    return DistanceComparison.from_sums(len(x), shift_x, shift_y, dx.sum(), dy.sum(), (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum(),
                                        x.min(), x.max(), y.min(), y.max())


def _uncorrelated():
    """float32 columns of a small clade whose covariance is almost nothing: one y moved until cov is below 1e-6 of
    sqrt(var_x var_y), as linked seed 2 case 3 draws it (six pairs, cov 6.6e-9 beside variances of 6.1 and 0.014)"""
    import numpy as np
    rng = np.random.default_rng(6)
    x = (7.0 + 2.5 * rng.standard_normal(15)).astype(np.float32).astype(np.float64)
    y = (1.0 + 0.1 * rng.standard_normal(15)).astype(np.float32).astype(np.float64)
    for _ in range(4):      # cov is linear in y[3]; the float32 rounding of y[3] leaves a remainder
        y[3] = np.float32(y[3] - np.cov(x, y, bias=True)[0, 1] * len(x) / (x[3] - x.mean()))
    return x, y


def test_the_derived_bound_of_a_clade_row_on_a_covariance_near_zero():
    """fuzz_compare._derived_moments, which the GPU sessions take only where _check_row's 1e-10 relative of var or cov is
    missed.  On columns whose covariance is a millionth of sqrt(var_x var_y) a correct float64 record passes; one whose
    covariance or variance is off by a third of the bound (3e-10 of the raw moments about the shift) passes, one off by three
    times the bound does not, nor does one with a sum outside its own bar, another r, or another maximum."""
    from dataclasses import replace
    import numpy as np
    x, y = _uncorrelated()
    c = _record(x, y, x[0], y[0])
    raw_x, raw_y = ((x - x[0]) ** 2).mean(), ((y - y[0]) ** 2).mean()
    scale = np.sqrt(raw_x * raw_y)
    assert abs(np.cov(x, y, bias=True)[0, 1]) < 1e-6 * np.sqrt(np.var(x) * np.var(y))
    assert fuzz_compare._derived_moments(c, c.pearson_r, x, y) is None
    assert fuzz_compare._derived_moments(replace(c, cov=c.cov + 1e-10 * scale), c.pearson_r, x, y) is None
    assert fuzz_compare._derived_moments(replace(c, cov=c.cov + 9e-10 * scale), c.pearson_r, x, y) is not None
    assert fuzz_compare._derived_moments(replace(c, var_x=c.var_x + 1e-10 * raw_x), c.pearson_r, x, y) is None
    assert fuzz_compare._derived_moments(replace(c, var_x=c.var_x + 9e-10 * raw_x), c.pearson_r, x, y) is not None
    assert fuzz_compare._derived_moments(replace(c, sxy=c.sxy + 1e-9 * len(x) * scale), c.pearson_r, x, y) is not None
    assert fuzz_compare._derived_moments(c, c.pearson_r + 1e-8, x, y) is not None
    assert fuzz_compare._derived_moments(replace(c, max_x=c.max_x + 1e-7), c.pearson_r, x, y) is not None


def test_the_derived_bound_of_a_merge_on_a_nearly_constant_column():
    """fuzz_compare._merge_bars: two halves summed about their own first pairs and merged, against the whole about its own:
    accepted (by the strict bar or by 1e-12 of the raw moment), a merged variance off by 1e-13 of the raw moment too, one
    off by 1e-11 of it not; on an ordinary column the strict bar alone decides and the fallback is not taken."""
    from dataclasses import replace
    from suchtree_amd.compare import DistanceComparison
    x, y = _nearly_constant()
    n, cut = len(x), 1500
    full = _record(x, y, x[:4096].mean(), y[:4096].mean())
    merged = DistanceComparison.merge(_record(x[:cut], y[:cut], x[0], y[0]), _record(x[cut:], y[cut:], x[cut], y[cut]))
    raw = full.sxx / n
    assert fuzz_compare._merge_bars(merged, full, n)[0] is None
    bad, derived = fuzz_compare._merge_bars(replace(merged, var_x=merged.var_x + 1e-13 * raw), full, n)
    assert bad is None
    bad, derived = fuzz_compare._merge_bars(replace(merged, var_x=merged.var_x + 1e-11 * raw), full, n)
    assert bad is not None and "var_x" in derived
    u = y      # an ordinary column on both sides
    whole = _record(u, u[::-1].copy(), u[:4096].mean(), u[::-1][:4096].mean())
    halves = DistanceComparison.merge(_record(u[:cut], u[::-1][:cut], u[0], u[-1]), _record(u[cut:], u[::-1][cut:], u[cut], u[::-1][cut]))
    assert fuzz_compare._merge_bars(halves, whole, n) == (None, [])
    assert fuzz_compare._merge_bars(replace(halves, var_x=halves.var_x * (1 + 1e-11)), whole, n)[0] is not None
