"""The plain float64 reference of the compare path's moments records, and the bars the GPU's records are held to: no GPU
and no library call but DistanceComparison's arithmetic on the finished sums.

_Sums          float64 sums of one pair range about a given shift, block by block, and the int64 np.histogram2d
_check_shift   the shift rule of k_pair_shift restated
_rel           the relative difference all bars are written in

tests/test_gpu_reductions.py, where these were written, and tests/fuzz_compare.py use them."""
import numpy as np

from suchtree_amd.compare import DistanceComparison

SHIFT_PAIRS = 4096                   # kernels_compare.h: kCmpShiftPairs


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


class _Sums:
    """float64 sums of one pair range about a given shift, fed block by block (host memory stays bounded by a block),
    and the int64 histogram over fixed edges."""

    def __init__(self, shift_x, shift_y, edges=None):
        self.cx, self.cy, self.edges = shift_x, shift_y, edges
        self.n, self.sx, self.sy, self.sxx, self.syy, self.sxy = 0, 0.0, 0.0, 0.0, 0.0, 0.0
        self.min_x = self.min_y = np.inf
        self.max_x = self.max_y = -np.inf
        self.hist = None if edges is None else np.zeros((len(edges[0]) - 1, len(edges[1]) - 1), np.int64)

    def add(self, x, y):
        dx, dy = x - self.cx, y - self.cy
        self.n += len(x)
        self.sx += dx.sum()
        self.sy += dy.sum()
        self.sxx += (dx * dx).sum()
        self.syy += (dy * dy).sum()
        self.sxy += (dx * dy).sum()
        self.min_x, self.max_x = min(self.min_x, x.min()), max(self.max_x, x.max())
        self.min_y, self.max_y = min(self.min_y, y.min()), max(self.max_y, y.max())
        if self.edges is not None:
            self.hist += np.histogram2d(x, y, bins=self.edges)[0].astype(np.int64)

    def check(self, m, hist=None):
        """The bars of _check_moments on the sums; the histogram exactly."""
        assert m.n == self.n
        for got, want in ((m.sxx, self.sxx), (m.syy, self.syy), (m.sxy, self.sxy)):
            assert _rel(got, want) < 1e-10 or abs(got - want) < 1e-12, (got, want)
        assert abs(m.sx - self.sx) <= 1e-10 * np.sqrt(self.n * m.sxx) and abs(m.sy - self.sy) <= 1e-10 * np.sqrt(self.n * m.syy)
        assert (m.min_x, m.max_x, m.min_y, m.max_y) == (self.min_x, self.max_x, self.min_y, self.max_y)
        got = DistanceComparison.from_moments(m)
        want = DistanceComparison.from_sums(self.n, self.cx, self.cy, self.sx, self.sy, self.sxx, self.syy, self.sxy,
                                            self.min_x, self.max_x, self.min_y, self.max_y)
        for k in ("mean_x", "mean_y", "var_x", "var_y", "cov", "pearson_r"):
            g, w = getattr(got, k), getattr(want, k)
            assert (np.isnan(g) and np.isnan(w)) or _rel(g, w) < 1e-10 or abs(g - w) < 1e-12, (k, g, w)
        if self.edges is not None:
            assert np.array_equal(hist, self.hist)


def _check_shift(m, x, y):
    """k_pair_shift: the mean of the call's first min(n, kCmpShiftPairs) pairs, 0 where that is not finite."""
    for got, head in ((m.shift_x, x[:SHIFT_PAIRS]), (m.shift_y, y[:SHIFT_PAIRS])):
        want = head.mean()
        want = want if np.isfinite(want) else 0.0
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
