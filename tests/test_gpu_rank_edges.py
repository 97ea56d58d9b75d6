"""The exact rank kernels (kernels_ranks.h; RankState and the Rank*Reduce passes of host_compare.h) at their arithmetic and
layout edges.  Realistic trees give a handful of adjacent positive key buckets, tie groups of a few thousand and sums
that barely pass 64 bits; here

A  arbitrary float32 columns reach the kernels: negative keys, subnormals either side of zero (buckets 2047 | 2048), the
   infinities and +-FLT_MAX (the lowest and highest buckets a value can fall in), heavy ties, all-distinct and constant
   columns, n = 1, 2, 3, 5 (no quad, only the n & 3 tail) and 8193;
B  values sit on the lane (16 counters), wave (1024) and scan-block (4096) edges of the count tables, at the last counter
   of a bucket and the first of the next, with multiplicities around 64 and 4096, in 1536 scan blocks;
C  a NaN on either side, in the first pair and in the last pair of a tail chunk;
D  the triangle over the 16384 leaves of a perfect tree with unit branch lengths: 14 tie groups of up to 2^26 pairs, tie
   sums of 79 bits, Sxy below -2^64;
(E, the same over 65536 leaves -- 2 147 450 880 pairs, the largest call the path takes, one counter holding 2^30 -- gave the
   analytic sums in all three modes but takes 16.4 s a mode on the MI355X, so it is not in the suite: LAB_NOTES.md.)

How a column gets there: the distance of the pair (node, its parent) is the node's branch length bit for bit, so a random
binary tree whose branch lengths are the column, with the child -> parent pairs in either order, delivers it; every case
first asserts that distances_host returns the column on those pairs.  The one float32 that does not survive is -0.0 (it
comes back as +0.0): -0.0 stays a host-only case (tests/test_spearman_host.py).

References: rank_sums (np.unique counts in Python integers) and perfect_tree_sums (analytic) of tests/rank_reference.py,
never the library's own st_spearman_host, which shares rank_key, rank_centered and rank_tie_term with the device.  Every
case: the same bytes with chunks of 8192 pairs and with the default chunk, the moments' bytes those of the plain compare call,
spearman_r within 1e-12 of scipy's, at most 64 occupied buckets per tree (256 MiB of counters) asserted before the launch."""
import math
import time
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
from scipy.stats import spearmanr

from conftest import assert_bits_equal
from rank_reference import (BUCKET_KEYS, LOW_BITS, bit_reverse, buckets_of, float_of, host_columns, key_of, perfect_tree_sums, rank_sums)
from suchtree_amd import SuchTree, synth
from suchtree_amd.compare import rank_fields

pytestmark = pytest.mark.gpu

MAX_BUCKETS = 64
FLT_MAX = np.float32(3.4028235e38)
N_A = 200_000                        # the non-root nodes of random_binary_tree(100_001)
SCAN_BLOCK = 4096                    # kernels_ranks.h: kRankScanBlock
CHUNKS = (8192, 0)


# ---- delivering a column ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _topology(n, seed):
    """(parent, the first n non-root nodes) of a random binary tree with at least n non-root nodes."""
    parent = np.asarray(synth.random_binary_tree((n + 3) // 2, seed=seed)[0])
    nodes = np.flatnonzero(parent >= 0)[:n].astype(np.int64)
    assert len(nodes) == n
    return parent, nodes


class _Injected:
    """A tree whose non-root branch lengths are `column`, and the child -> parent pairs that read them back (odd rows as
    parent -> child)."""

    def __init__(self, column, seed):
        self.column = np.ascontiguousarray(column, dtype=np.float32)
        assert not (np.signbit(self.column) & (self.column == 0)).any()      # -0.0 is not delivered
        parent, nodes = _topology(len(self.column), seed)
        distance = np.ones(len(parent), dtype=np.float32)
        distance[parent < 0] = 0.0
        distance[nodes] = self.column
        self.tree = SuchTree((parent, distance))
        self.dev = self.tree._device_tree()
        self.pairs = np.stack([nodes, parent[nodes].astype(np.int64)], axis=1)
        self.pairs[1::2] = self.pairs[1::2, ::-1]

    def reached(self, n=None):
        """The first n pairs' column, after asserting that the GPU's distances on them are the column bit for bit."""
        n = len(self.column) if n is None else n
        d, _ = self.dev.distances_host(self.pairs[:n])
        assert_bits_equal(d, self.column[:n].astype(np.float64), "injected column")
        finite = self.column[:n][~np.isnan(self.column[:n])]
        assert len(buckets_of(finite)) <= MAX_BUCKETS, len(buckets_of(finite))
        return self.column[:n]


def _same_sums(r, want):
    got = (int(r.n), int(r.n_nan), r.sxy, r.sxx, r.syy, int(r.distinct_x), int(r.distinct_y))
    assert got == tuple(want), [(k, g, w) for k, g, w in zip(want._fields, got, want) if g != w]


def _check_r(r, want, x=None, y=None, exact=None):
    """spearman_r of the sums r against scipy on the columns (or against `exact`, a Fraction of r^2's sign and size)."""
    got = rank_fields(r)["spearman_r"]
    if want.n < 2 or want.n_nan or want.sxx == 0 or want.syy == 0:
        assert math.isnan(got)
        return
    rs = float(exact) if exact is not None else spearmanr(x.astype(np.float64), y.astype(np.float64))[0]
    print("spearman_r %.17g, reference %.17g, difference %.3g" % (got, rs, got - rs))
    assert abs(got - rs) < 1e-12


def _check_pairs(X, Y, n=None):
    """Groups A to C: the ranks of the first n injected pairs of X against those of Y."""
    x, y = X.reached(n), Y.reached(n)
    px, py = X.pairs[:len(x)], Y.pairs[:len(y)]
    want = rank_sums(x, y)
    m0, _ = X.dev.compare_pairs_host(Y.dev, px, py)
    seen = []
    for chunk in CHUNKS:
        m, r = X.dev.compare_pairs_ranks_host(Y.dev, px, py, chunk_pairs=chunk)
        _same_sums(r, want)
        assert bytes(m) == bytes(m0)
        seen.append(bytes(r))
    assert len(set(seen)) == 1
    _check_r(r, want, x, y)
    return want, r


# ---- A: injected columns ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _columns_a():
    host = host_columns()
    heavy, mixed = host["heavy ties vs mixed zeros"]
    mixed = np.where(mixed == 0, np.float32(0.0), mixed).astype(np.float32)
    sub = host["subnormals vs wide range"][0]
    rng = np.random.default_rng(51)
    # the host file's wide range, confined: 60 buckets drawn from all that hold finite values (8: -FLT_MAX .. 4087: FLT_MAX)
    chosen = np.sort(rng.choice(np.arange(8, 4088), 60, replace=False))
    keys = (chosen[rng.integers(0, 60, N_A)] << LOW_BITS) | rng.integers(0, BUCKET_KEYS, N_A)
    wide = float_of(keys)
    assert np.isfinite(wide).all() and (wide < 0).sum() > N_A // 4 and (wide > 0).sum() > N_A // 4
    wide_inf = wide.copy()
    wide_inf[rng.random(N_A) < 0.01] = np.inf
    extremes = wide.copy()
    pick = rng.random(N_A)
    for i, v in enumerate((-np.inf, -FLT_MAX, FLT_MAX, np.inf)):
        extremes[(pick >= 0.02 * i) & (pick < 0.02 * (i + 1))] = v
    assert [int(b) for b in buckets_of(extremes)[[0, 1, -2, -1]]] == [7, 8, 4087, 4088]
    assert [int(b) for b in buckets_of(sub)] == [2047, 2048]
    distinct = float_of(int(key_of(np.float32([1.0]))[0]) + 5 * rng.permutation(N_A))
    keys = 0x80000000 - N_A // 2 + rng.permutation(N_A)      # all distinct: subnormals of both signs and +0.0
    keys[keys < 0x80000000] -= 1                             # (0x7fffffff is no value's key: it would be -0.0's)
    across_zero = float_of(keys)
    assert len(np.unique(distinct)) == len(np.unique(across_zero)) == N_A and (across_zero < 0).sum() == N_A // 2
    cols = {"heavy": heavy, "mixed": mixed, "sub": sub, "wide": wide, "wide_inf": wide_inf, "extremes": extremes,
            "distinct": distinct, "across_zero": across_zero, "constant": np.full(N_A, 0.75, np.float32)}
    assert all(c.dtype == np.float32 and len(c) == N_A for c in cols.values())
    return cols


@lru_cache(maxsize=None)
def _injected_a(name, side):
    return _Injected(_columns_a()[name], seed=61 + side)      # tree X and tree Y: a topology each


CASES_A = {
    "heavy ties vs ties and zeros": ("heavy", "mixed"),
    "both signs in 61 buckets with inf vs heavy ties": ("wide_inf", "heavy"),
    "subnormals around zero vs both signs": ("sub", "wide"),
    "infinities and FLT_MAX vs all distinct across zero": ("extremes", "across_zero"),
    "all distinct vs heavy ties": ("distinct", "heavy"),
    "all distinct vs all distinct": ("distinct", "across_zero"),
    "constant vs all distinct": ("constant", "distinct"),
}


@pytest.mark.parametrize("case", list(CASES_A))
def test_injected_columns(case):
    nx, ny = CASES_A[case]
    X, Y = _injected_a(nx, 0), _injected_a(ny, 1)
    want, _ = _check_pairs(X, Y)
    assert want.n == N_A and want.n_nan == 0
    if nx == "constant":
        assert want.sxx == 0 and want.distinct_x == 1
    if nx == "distinct":
        assert want.distinct_x == N_A and 3 * want.sxx == N_A ** 3 - N_A
    # the public call returns the same
    c = X.tree.compare_distances(Y.tree, pairs=(X.pairs, Y.pairs), spearman=True)
    assert (c.rank_sxy, c.rank_sxx, c.rank_syy, c.distinct_x, c.distinct_y) == want[2:]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8193])
def test_injected_columns_at_small_n(n):
    want, _ = _check_pairs(_injected_a("extremes", 0), _injected_a("sub", 1), n)
    assert want.n == n
    want, _ = _check_pairs(_injected_a("wide", 1), _injected_a("heavy", 0), n)
    assert want.n == n


# ---- B: the layout of the count tables ---------------------------------------------------------------------------------
POSITIONS = (0, 15, 16, 1023, 1024, 4095, 4096, BUCKET_KEYS - 1)
MULTIPLICITIES = (1, 2, 63, 64, 65, 4097)


@lru_cache(maxsize=None)
def _layout_column():
    """Every position of POSITIONS in a bucket of negative and in a bucket of positive values, then counter 0 of the next
    bucket (a slot change after the bucket's last counter) and of buckets far above: 6 occupied buckets, 1536 scan blocks,
    so that one lane of k_rank_scan_blocks carries an offset over several blocks and over a whole empty bucket."""
    negative, positive = int(key_of(np.float32([-3.0]))[0]) >> LOW_BITS, int(key_of(np.float32([3.0]))[0]) >> LOW_BITS
    keys = [(b << LOW_BITS) | p for b in (negative, positive) for p in POSITIONS]
    keys += [(negative + 1) << LOW_BITS, (positive + 1) << LOW_BITS, (positive + 300) << LOW_BITS, ((positive + 300) << LOW_BITS) | 17]
    keys += [((positive + 700) << LOW_BITS) | 4096]
    keys = np.array(sorted(keys), dtype=np.int64)
    mult = np.array([MULTIPLICITIES[(i * 5 + i // 6) % 6] for i in range(len(keys))], dtype=np.int64)
    for edge in (15, 1023, 4095, BUCKET_KEYS - 1):      # either side of every edge, some pair of counters holds more than one value
        at = np.flatnonzero((keys & (BUCKET_KEYS - 1)) == edge)
        assert len(at) == 2 and (mult[at] + mult[at + 1] > 2).all()
    assert set(mult) == set(MULTIPLICITIES)
    column = np.repeat(float_of(keys), mult)
    buckets = buckets_of(column)
    assert len(buckets) == 6 and len(buckets) * (BUCKET_KEYS // SCAN_BLOCK) > 1024 and (column < 0).any() and (column > 0).any()
    assert np.array_equal(np.unique(key_of(column)), keys)
    return column[np.random.default_rng(52).permutation(len(column))]


@pytest.mark.parametrize("other", ["itself", "its reverse", "a permutation"])
def test_table_layout_edges(other):
    col = _layout_column()
    y = {"itself": col, "its reverse": col[::-1], "a permutation": col[np.random.default_rng(53).permutation(len(col))]}[other]
    want, r = _check_pairs(_Injected(col, 63), _Injected(y, 64))
    assert want.distinct_x == want.distinct_y == 21 and want.sxx == want.syy
    if other == "itself":
        assert want.sxy == want.sxx and rank_fields(r)["spearman_r"] == 1.0


# ---- C: NaN ----------------------------------------------------------------------------------------------------------
N_C = 8192 * 3 + 1


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("side", ["x", "y", "both"])
def test_nan_pairs(side, where):
    rng = np.random.default_rng(54)
    x = rng.integers(-50, 50, N_C).astype(np.float32) * np.float32(0.25)
    y = (1.0 + rng.random(N_C)).astype(np.float32)              # [1, 2): 8 buckets
    at = 0 if where == "first" else N_C - 1
    if side in ("x", "both"):
        x[[at, 5000, 5001]] = np.nan
    if side in ("y", "both"):
        y[[at, 5001, 20000]] = np.nan
    n_nan = {"x": 3, "y": 3, "both": 4}[side]
    X, Y = _Injected(x, 65), _Injected(y, 66)
    want, r = _check_pairs(X, Y)
    assert tuple(want) == (N_C, n_nan, 0, 0, 0, 0, 0)
    assert math.isnan(rank_fields(r)["spearman_r"])
    c = X.tree.compare_distances(Y.tree, pairs=(X.pairs, Y.pairs), spearman=True)
    assert math.isnan(c.spearman_r) and (c.rank_sxy, c.rank_sxx, c.rank_syy, c.distinct_x, c.distinct_y) == (0, 0, 0, 0, 0)
    # without the NaN pairs the same call gives sums
    keep = ~(np.isnan(x) | np.isnan(y))
    assert keep.sum() == N_C - n_nan
    _, r = X.dev.compare_pairs_ranks_host(Y.dev, X.pairs[keep], Y.pairs[keep], chunk_pairs=8192)
    _same_sums(r, rank_sums(x[keep], y[keep]))


# ---- D: the high words ---------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _perfect(L, length):
    parent, distance = synth.balanced_tree(L)
    distance = np.where(parent < 0, distance, np.float32(length)).astype(np.float32)
    return SuchTree((parent, distance))


def _perfect_case(L, mode):
    """(tree X, tree Y, ids_x, ids_y): leaf k has id 2 k."""
    ids = 2 * np.arange(1 << L, dtype=np.int64)
    X = _perfect(L, 1.0)
    if mode == "negated":
        return X, _perfect(L, -1.0), ids, ids
    return X, X, ids, 2 * bit_reverse(np.arange(1 << L), L) if mode == "bitreversed" else ids


def _exact_r(want):
    """Sxy / sqrt(Sxx Syy), scipy's definition on the midranks, to well below 1e-12 without a sort of 10^8 pairs."""
    scale = 10 ** 40
    root = math.isqrt(want.sxx * want.syy * scale * scale)
    return Fraction(want.sxy * scale, root)


def _check_perfect(L, mode, chunks):
    X, Y, ids_x, ids_y = _perfect_case(L, mode)
    want = perfect_tree_sums(L, mode)
    assert want.distinct_x == want.distinct_y == L <= MAX_BUCKETS       # L distances, at most a bucket each
    dx, dy = X._device_tree(), Y._device_tree()
    m0, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    seen = []
    for chunk in chunks:
        t0 = time.perf_counter()
        m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, chunk_pairs=chunk)
        print("L %d %s chunk_pairs %d: %.3f s" % (L, mode, chunk, time.perf_counter() - t0))
        _same_sums(r, want)
        assert bytes(m) == bytes(m0)
        seen.append(bytes(r))
    assert len(set(seen)) == 1
    assert m.n == want.n and (m.min_x, m.max_x) == (2.0, 2.0 * L)
    assert (m.min_y, m.max_y) == ((-2.0 * L, -2.0) if mode == "negated" else (2.0, 2.0 * L))
    _check_r(r, want, exact=_exact_r(want))
    if mode != "bitreversed":
        assert rank_fields(r)["spearman_r"] == (1.0 if mode == "identity" else -1.0)
        assert abs(want.sxy) == want.sxx
    else:
        assert r.sxy_hi < -1 and r.sxx_hi > 0                             # Sxy below -2^64
    return r


@pytest.mark.parametrize("mode", ["identity", "negated", "bitreversed"])
def test_high_words_on_a_perfect_tree_of_16384_leaves(mode):
    _check_perfect(14, mode, CHUNKS)


def test_sub_range_of_the_perfect_triangle_that_splits_chunks():
    X, Y, ids_x, ids_y = _perfect_case(14, "bitreversed")
    dx, dy = X._device_tree(), Y._device_tree()
    k0, kc = 100_000_000 + 12345, 8192 * 5 + 3          # begins and ends inside a chunk of 8192
    x = dx.triangle_host(ids_x, k0, kc)[0].astype(np.float32)
    y = dy.triangle_host(ids_y, k0, kc)[0].astype(np.float32)
    i = (1 + np.sqrt(1 + 8 * np.arange(k0, k0 + kc, dtype=np.float64))) // 2      # pair k = (ids[j], ids[i]), k = i (i - 1) / 2 + j
    i = i.astype(np.int64)
    j = np.arange(k0, k0 + kc, dtype=np.int64) - i * (i - 1) // 2
    assert (j >= 0).all() and (j < i).all()
    assert np.array_equal(x, np.float32([2 * int(d).bit_length() for d in i ^ j]))
    want = rank_sums(x, y)
    assert want.n == kc and want.distinct_x > 3 and want.distinct_y > 3
    m0, _ = dx.compare_triangle_host(dy, ids_x, ids_y, k0, kc)
    seen = []
    for chunk in CHUNKS:
        m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, k0, kc, chunk_pairs=chunk)
        _same_sums(r, want)
        assert bytes(m) == bytes(m0)
        seen.append(bytes(r))
    assert len(set(seen)) == 1
    _check_r(r, want, x, y)

