"""References for the exact Kendall tau-b counts, independent of the library: no GPU, no suchtree_amd code.

brute_counts      the counts of include/suchtree_hip.h: st_kendall_counts by comparing every pair of pairs, O(n^2) in numpy
tie_sum           sum of t (t - 1) / 2 over the tie groups of one column, from np.unique counts
tau_b             tau-b from the counts in Python integers and one float division
heavy_columns     seeded columns of few distinct values: tie groups far longer than any tile
"""
from collections import namedtuple

import numpy as np

KendallRef = namedtuple("KendallRef", "n n_nan discordant ties_x ties_y ties_xy")

BLOCK = 512      # rows of the n x n comparison held at a time


def brute_counts(x, y):
    """KendallRef(n, n_nan, discordant, ties_x, ties_y, ties_xy) of two float32 columns, every field a Python int, by
    looking at every {i, j}.  A NaN on either side of any pair: n_nan counts such pairs and every count is 0."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert x.ndim == 1 and x.shape == y.shape
    n = len(x)
    n_nan = int((np.isnan(x) | np.isnan(y)).sum())
    if n_nan or n == 0:
        return KendallRef(n, n_nan, 0, 0, 0, 0)
    dis = tx = ty = txy = 0
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        later = np.arange(n)[None, :] > np.arange(lo, hi)[:, None]      # each {i, j} once: j > i
        with np.errstate(invalid="ignore"):                             # (inf - inf is never formed: signs of comparisons)
            sx = np.sign((x[None, :] > x[lo:hi, None]).astype(np.int8) - (x[None, :] < x[lo:hi, None]).astype(np.int8))
            sy = np.sign((y[None, :] > y[lo:hi, None]).astype(np.int8) - (y[None, :] < y[lo:hi, None]).astype(np.int8))
        dis += int(((sx * sy < 0) & later).sum())
        tx += int(((sx == 0) & later).sum())
        ty += int(((sy == 0) & later).sum())
        txy += int(((sx == 0) & (sy == 0) & later).sum())
    return KendallRef(n, 0, dis, tx, ty, txy)


def tie_sum(v):
    _, t = np.unique(np.asarray(v, dtype=np.float32), return_counts=True)      # (-0.0 == +0.0: one group)
    return sum(int(c) * (int(c) - 1) // 2 for c in t)


def tau_b(ref):
    n0 = ref.n * (ref.n - 1) // 2
    fx, fy = n0 - ref.ties_x, n0 - ref.ties_y
    if ref.n < 2 or ref.n_nan or fx == 0 or fy == 0:
        return float("nan")
    con = n0 - ref.ties_x - ref.ties_y + ref.ties_xy - ref.discordant
    return (con - ref.discordant) / float(np.sqrt(float(fx) * float(fy)))


def heavy_columns(n, seed, values=5):
    """Two float32 columns of n values drawn from `values` distinct ones (both zeros among them), weakly related."""
    rng = np.random.default_rng(seed)
    pool = np.float32([-0.0, 0.0, 1.5, -2.0, np.inf, 3.0e-41, -7.25])[:values + 1]
    x = pool[rng.integers(0, len(pool), n)]
    y = np.where(rng.random(n) < 0.5, x, pool[rng.integers(0, len(pool), n)]).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y)
