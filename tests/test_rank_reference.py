"""The references of tests/rank_reference.py against other references: rank_sums against scipy's midranks, the analytic
sums of a perfect tree against brute force over every pair and against the figures worked out with the oracle, the numpy
key against the order of the floats.  No GPU and no library code."""
import numpy as np
import pytest

from rank_reference import (MODES, bit_reverse, buckets_of, float_of, host_columns, key_of, perfect_tree_levels, perfect_tree_sums,
                            perfect_tree_ties, rank_sums, scipy_midrank_sums, tie_identity)

SMALL = 3000      # scipy_midrank_sums keeps a Python int per value


@pytest.mark.parametrize("case", list(host_columns()))
def test_rank_sums_equal_scipy_midranks(case):
    x, y = host_columns()[case]
    x, y = x[:SMALL], y[:SMALL]
    r = rank_sums(x, y)
    assert all(type(v) is int for v in r)
    assert (r.n, r.n_nan) == (len(x), 0)
    assert (r.sxy, r.sxx, r.syy) == scipy_midrank_sums(x, y)
    assert (r.sxx, r.syy) == (tie_identity(x), tie_identity(y))
    assert (r.distinct_x, r.distinct_y) == (len(np.unique(x)), len(np.unique(y)))


def test_rank_sums_at_full_length_keep_the_tie_identity_and_the_symmetries():
    x, y = host_columns()["wide range with inf vs heavy ties"]
    r = rank_sums(x, y)
    assert r.n == 200_000 and (r.sxx, r.syy) == (tie_identity(x), tie_identity(y))
    assert rank_sums(y, x) == r._replace(sxx=r.syy, syy=r.sxx, distinct_x=r.distinct_y, distinct_y=r.distinct_x)
    assert rank_sums(x, -y).sxy == -r.sxy and rank_sums(x, x).sxy == r.sxx
    assert r.sxy ** 2 <= r.sxx * r.syy


def test_rank_sums_nan_empty_and_negative_zero():
    x = np.float32([1, 2, np.nan, 4, 5])
    y = np.float32([np.nan, 1, np.nan, 3, 2])
    assert rank_sums(x, y) == (5, 2, 0, 0, 0, 0, 0)
    assert rank_sums(x[:2], y[1:3]) == (2, 1, 0, 0, 0, 0, 0)
    assert rank_sums(np.zeros(0, np.float32), np.zeros(0, np.float32)) == (0, 0, 0, 0, 0, 0, 0)
    assert rank_sums(np.float32([7]), np.float32([-7])) == (1, 0, 0, 0, 0, 1, 1)
    z = rank_sums(np.float32([0.0, -0.0, 1.0, -1.0]), np.float32([-0.0, 0.0, 2.0, -2.0]))
    assert z.distinct_x == z.distinct_y == 3 and z.sxy == z.sxx == z.syy == (4 ** 3 - 4 - 6) // 3
    c = rank_sums(np.float32([3, 3, 3, 3]), np.float32([1, 2, 3, 4]))
    assert (c.sxy, c.sxx, c.syy, c.distinct_x, c.distinct_y) == (0, 0, 20, 1, 4)


@pytest.mark.parametrize("mode", MODES)
def test_perfect_tree_sums_equal_brute_force_over_all_2016_pairs(mode):
    L = 6
    rows, cols = np.tril_indices(1 << L, -1)
    assert len(rows) == 2016

    def distance(i, j, length):      # leaves i, j of the perfect tree: bit_length(i ^ j) edges up and as many down
        return np.float32([2 * length * int(d).bit_length() for d in i ^ j])
    x = distance(cols, rows, 1.0)
    if mode == "identity":
        y = x
    elif mode == "negated":
        y = distance(cols, rows, -1.0)
    else:
        rev = bit_reverse(np.arange(1 << L), L)
        assert sorted(rev) == list(range(1 << L)) and rev[1] == 32 and rev[3] == 48
        y = distance(rev[cols], rev[rows], 1.0)
    want = rank_sums(x, y)
    assert perfect_tree_sums(L, mode) == want
    assert (want.sxy, want.sxx, want.syy) == scipy_midrank_sums(x, y)
    lx, ly = perfect_tree_levels(L, mode)      # every XOR value 2^(L-1) times: the table of the levels is the table of the pairs
    pairs = sorted(zip((x / 2).astype(int), (np.abs(y) / 2).astype(int)))
    assert pairs == sorted(zip(np.repeat(lx, 32), np.repeat(ly, 32)))


# worked out with the oracle's distances on the CPU when these tests were planned
TABLE = {
    14: dict(n=134_209_536, sxx=690667189119954890784768, sxy_bitreversed=-147384800855571038208,
             ties=345407377032672522018816, tie_bits=79, largest=2 ** 26),
    16: dict(n=2_147_450_880, sxx=2829426119230678899087114240, sxy_bitreversed=-151060387184423146094592,
             ties=1414788616326143857112678400, tie_bits=91, largest=2 ** 30),
}


@pytest.mark.parametrize("L", sorted(TABLE))
def test_perfect_tree_sums_reproduce_the_planned_figures(L):
    t = TABLE[L]
    same, neg, rev = (perfect_tree_sums(L, m) for m in MODES)
    for r in (same, neg, rev):
        assert (r.n, r.n_nan, r.sxx, r.syy, r.distinct_x, r.distinct_y) == (t["n"], 0, t["sxx"], t["sxx"], L, L)
    assert t["n"] <= 2 ** 31 - 1
    assert same.sxy == t["sxx"] and neg.sxy == -t["sxx"] and rev.sxy == t["sxy_bitreversed"]
    ties, largest = perfect_tree_ties(L)
    assert (ties, ties.bit_length(), largest) == (t["ties"], t["tie_bits"], t["largest"])
    assert 3 * t["sxx"] == t["n"] ** 3 - t["n"] - ties
    # what the GPU tests reach with them: both high words of the sums, and the sign of Sxy's
    assert t["sxx"] >> 64 > 0 and ties >> 64 > 0 and rev.sxy < -2 ** 64


def test_key_and_float_are_inverses_and_the_key_is_monotone():
    rng = np.random.default_rng(41)
    v = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v = v[np.isfinite(v)]
    v = np.concatenate([v, np.float32([np.inf, -np.inf, 0.0, 3.4028235e38, -3.4028235e38, 1e-45, -1e-45, 1.1754944e-38])])
    v = np.unique(v[~((v == 0) & np.signbit(v))])      # sorted, distinct, no -0.0
    k = key_of(v)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(float_of(k).view(np.uint32), v.view(np.uint32))
    keys = rng.integers(key_of(np.float32([-np.inf]))[0], int(key_of(np.float32([np.inf]))[0]) + 1, 100_000, dtype=np.int64)
    keys = keys[keys != 0x7fffffff]      # the one hole: -0.0 shares +0.0's key
    assert np.array_equal(key_of(float_of(keys)), keys.astype(np.uint32))
    assert np.signbit(float_of(np.uint32([0x7fffffff])))[0] and float_of(np.uint32([0x7fffffff]))[0] == 0
    order = np.argsort(keys, kind="stable")
    assert (np.diff(float_of(keys[order]).astype(np.float64)) >= 0).all()
    # the ends and the middle of the key space, and -0.0
    assert [int(b) for b in buckets_of(np.float32([-np.inf, -3.4028235e38, -1e-45, 0.0, 1e-45, 3.4028235e38, np.inf]))] == [7, 8, 2047, 2048, 4087, 4088]
    assert key_of(np.float32([-0.0]))[0] == key_of(np.float32([0.0]))[0] == 0x80000000
    assert not np.signbit(float_of(np.uint32([0x80000000])))[0]
    assert int(key_of(np.float32([1.0]))[0]) == 0xBF800000 and int(key_of(np.float32([-1.0]))[0]) == 0x407FFFFF
