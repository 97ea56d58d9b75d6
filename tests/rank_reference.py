"""References for the exact Spearman rank sums, independent of the library: no GPU, no suchtree_amd code.

rank_sums            the sums of include/suchtree_hip.h: st_rank_sums from np.unique counts, in Python integers
scipy_midrank_sums   the same sums from scipy.stats.rankdata (small n: it keeps one Python int per value)
tie_identity         Sxx from the tie groups alone
key_of / float_of    the order-preserving uint32 key of a float32 (rank_plan.h: rank_key) restated in numpy, and back
perfect_tree_sums    the sums of the triangle over all leaves of a perfect tree with unit branch lengths, analytically
host_columns         the float32 columns of tests/test_spearman_host.py
"""
from collections import namedtuple

import numpy as np
from scipy.stats import rankdata

RankRef = namedtuple("RankRef", "n n_nan sxy sxx syy distinct_x distinct_y")

TOP_BITS, LOW_BITS = 12, 20          # rank_plan.h: kRankTopBits, kRankLowBits
BUCKET_KEYS = 1 << LOW_BITS
MODES = ("identity", "negated", "bitreversed")


def _centered(v, n):
    """(a per distinct value as int64, index of each element's distinct value, counts): a = 2 less + count - n."""
    _, inv, cnt = np.unique(v.astype(np.float64), return_inverse=True, return_counts=True)      # (-0.0 == +0.0: one group)
    cnt = cnt.astype(np.int64)
    less = np.cumsum(cnt) - cnt
    return 2 * less + cnt - n, inv.reshape(-1).astype(np.int64), cnt


def _dot(weight, a, b):
    """sum of weight * a * b in Python integers (int64 arrays in: |a|, |b| < 2^31, but the sum passes 2^64)."""
    return int((weight.astype(object) * a.astype(object) * b.astype(object)).sum()) if len(weight) else 0


def rank_sums(x, y):
    """RankRef(n, n_nan, Sxy, Sxx, Syy, distinct_x, distinct_y) of two float32 columns, every field a Python int.
    A NaN on either side of any pair: n_nan counts such pairs and every sum and distinct count is 0."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert x.ndim == 1 and x.shape == y.shape
    n = len(x)
    n_nan = int((np.isnan(x) | np.isnan(y)).sum())
    if n_nan or n == 0:
        return RankRef(n, n_nan, 0, 0, 0, 0, 0)
    ax, ix, cx = _centered(x, n)
    ay, iy, cy = _centered(y, n)
    cell, cells = np.unique(ix * len(cy) + iy, return_counts=True)      # the contingency table's occupied cells
    sxy = _dot(cells.astype(np.int64), ax[cell // len(cy)], ay[cell % len(cy)])
    return RankRef(n, 0, sxy, _dot(cx, ax, ax), _dot(cy, ay, ay), len(cx), len(cy))


def scipy_midrank_sums(x, y):
    """(Sxy, Sxx, Syy) as Python ints from scipy's midranks: a = 2 rank - (n + 1) is an integer."""
    n = len(x)
    a2 = 2 * rankdata(x.astype(np.float64), "average") - (n + 1)
    b2 = 2 * rankdata(y.astype(np.float64), "average") - (n + 1)
    assert np.array_equal(a2, np.rint(a2)) and np.array_equal(b2, np.rint(b2))
    a, b = [int(v) for v in a2], [int(v) for v in b2]
    return sum(p * q for p, q in zip(a, b)), sum(p * p for p in a), sum(q * q for q in b)


def tie_identity(v):
    n = len(v)
    _, t = np.unique(v, return_counts=True)      # (-0.0 == +0.0: one group)
    ties = sum(int(c) ** 3 - int(c) for c in t)
    assert (n ** 3 - n - ties) % 3 == 0
    return (n ** 3 - n - ties) // 3


def key_of(v):
    """uint32 keys whose unsigned order is the order of the float32 values v (no NaN): -0.0 as +0.0, then the sign bit set
    on non-negative values and every bit flipped on negative ones."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    bits = np.where(bits == np.uint32(0x80000000), np.uint32(0), bits)
    return np.where(bits >> np.uint32(31) == 1, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def float_of(keys):
    """The float32 values of uint32 keys: key_of's inverse.  0x7fffffff is no value's key (it would be -0.0's, which shares
    +0.0's); every other key from -inf's 0x007fffff to +inf's 0xff800000 is one value's."""
    keys = np.asarray(keys).astype(np.uint32)
    bits = np.where(keys >> np.uint32(31) == 1, keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)
    return np.ascontiguousarray(bits).view(np.float32)


def buckets_of(v):
    """The occupied top-12-bit key buckets of a float32 column, ascending: 2^20 uint32 counters (4 MiB) each on the GPU."""
    return np.unique(key_of(v) >> np.uint32(LOW_BITS)).astype(np.int64)


def bit_reverse(k, bits):
    k = np.asarray(k, dtype=np.int64)
    out = np.zeros_like(k)
    for b in range(bits):
        out |= ((k >> b) & 1) << (bits - 1 - b)
    return out


def _bit_length(d):
    out = np.zeros_like(d)
    for b in range(63):
        out[d >> b > 0] = b + 1
    return out


def perfect_tree_levels(L, mode):
    """(x level, y level) int64 arrays over d = 1 .. 2^L - 1: in the triangle over the 2^L leaves of a perfect tree, leaf k
    at position k on the x side, every XOR value d = i ^ j occurs 2^(L-1) times, and the pair's distance with unit
    branch lengths is 2 * level, level = bit_length(d).  On the y side: `identity` the same leaves (the same level),
    `negated` the same leaves with every branch length -1.0 (distance -2 * level), `bitreversed` leaf bitreverse_L(k)
    at position k (level L - ctz(d))."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (MODES,))
    d = np.arange(1, 1 << L, dtype=np.int64)
    lx = _bit_length(d)
    return lx, L - (_bit_length(d & -d) - 1) if mode == "bitreversed" else lx.copy()      # (d & -d: the lowest set bit)


def perfect_tree_sums(L, mode):
    """RankRef of that triangle, from the L x L contingency table of the levels alone."""
    lx, ly = perfect_tree_levels(L, mode)
    each = 1 << (L - 1)                              # pairs per XOR value
    n = each * ((1 << L) - 1)
    table = [[0] * (L + 1) for _ in range(L + 1)]
    for cell, c in zip(*np.unique(lx * (L + 1) + ly, return_counts=True)):
        table[int(cell) // (L + 1)][int(cell) % (L + 1)] = int(c) * each
    cx = [sum(row) for row in table]
    cy = [sum(table[i][j] for i in range(L + 1)) for j in range(L + 1)]

    def centered(c, descending):
        a, less = [0] * (L + 1), 0
        for lvl in (range(L, 0, -1) if descending else range(1, L + 1)):
            a[lvl] = 2 * less + c[lvl] - n
            less += c[lvl]
        return a
    ax, ay = centered(cx, False), centered(cy, mode == "negated")      # (-2 * level: the deepest level ranks first)
    sxy = sum(table[i][j] * ax[i] * ay[j] for i in range(1, L + 1) for j in range(1, L + 1))
    sxx = sum(cx[i] * ax[i] ** 2 for i in range(1, L + 1))
    syy = sum(cy[j] * ay[j] ** 2 for j in range(1, L + 1))
    return RankRef(n, 0, sxy, sxx, syy, sum(c > 0 for c in cx), sum(c > 0 for c in cy))


def perfect_tree_ties(L):
    """(the tie sum of either side: sum of t^3 - t over the levels, the largest level's pair count) of that triangle."""
    counts = [(1 << (L - 1)) * (1 << (lvl - 1)) for lvl in range(1, L + 1)]
    return sum(t ** 3 - t for t in counts), max(counts)


def host_columns():
    """The (x, y) float32 columns of tests/test_spearman_host.py: ties, both zeros, a wide range with inf, subnormals."""
    rng = np.random.default_rng(31)
    n = 200_000
    heavy = rng.integers(-40, 40, n).astype(np.float32) * np.float32(0.125)
    zeros = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    mixed = np.where(rng.random(n) < 0.3, zeros, heavy).astype(np.float32)
    spread = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    spread[rng.random(n) < 0.01] = np.inf
    sub = (rng.integers(-1000, 1000, n).astype(np.float64) * 1.4e-45).astype(np.float32)      # subnormals, both signs
    distinct = rng.permutation(n).astype(np.float32)
    assert len(np.unique(distinct)) == n and (np.abs(sub[sub != 0]) < 1.2e-38).all() and np.signbit(mixed[mixed == 0]).any()
    return {
        "heavy ties vs mixed zeros": (heavy, mixed),
        "wide range with inf vs heavy ties": (spread, heavy),
        "subnormals vs wide range": (sub, spread),
        "all distinct vs all distinct": (distinct, rng.permutation(n).astype(np.float32)),
        "all distinct vs heavy ties": (distinct, heavy),
        "small": (heavy[:37], spread[:37]),
        "two": (np.float32([1, 2]), np.float32([5, -5])),
    }
