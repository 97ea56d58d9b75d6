"""Comparing two trees' distances over the same pairs, reduced on the GPU (SuchTree.compare_distances,
SuchLinkedTrees.linked_distances_summary; C ABI st_compare_triangle_host / st_compare_pairs_host), and their
topologies over the same quartets, counted on the GPU (SuchTree.compare_quartets; st_compare_quartets_*_host).

No counterpart in the reference: its comparison workflows (docs/examples/SuchTree_examples.md, "Comparing the
topologies of two large trees"; SuchLinkedTrees.linked_distances, MuchTree.pyx:2900-2934) bring every distance back
to the host and reduce it with numpy / scipy.  Here only the moments of the joint distribution and, if asked, an exact
2-D histogram leave the GPU.
"""
import math
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

__all__ = ["DistanceComparison", "CladeComparisons", "HommolaResult", "QuartetComparison", "SetDispersion", "SetUniFrac", "quartet_positions",
           "unifrac_from_depths", "MantelResult", "mantel", "Dendrogram", "TopologyTestResult", "linkage", "dendrogram_congruence"]


@dataclass(frozen=True)
class DistanceComparison:
    """Summary of n pairs' distances x (first tree) and y (second tree).

    Statistics are population ones (numpy's ``var`` / ``cov(..., bias=True)``); ``pearson_r`` is NaN when a variance is 0.
    ``hist`` is ``numpy.histogram2d(x, y, bins, range)[0]`` as int64 (None when no histogram was asked for), with
    ``xedges`` / ``yedges`` its edges.  ``n_leaves`` is the length of the id list whose pairs were compared (None for
    explicit pairs).  The raw sums -- ``sx`` = sum of (x - shift_x), ``sxx`` = sum of (x - shift_x)^2, ``sxy`` = sum of
    (x - shift_x)(y - shift_y), ... -- are kept so that results over disjoint pair ranges can be combined (:meth:`merge`).

    With ``spearman=True`` the call also ranks every pair: ``spearman_r`` is Spearman's rs of all n pairs (midranks, as
    ``scipy.stats.spearmanr``; NaN for a constant column, n < 2 or a NaN distance), computed from the exact integers
    ``rank_sxy`` = sum a b, ``rank_sxx`` = sum a^2, ``rank_syy`` = sum b^2 with a = 2 rank(x) - (n + 1), b likewise for y
    (Python ints: they do not depend on reduction order, chunking or device); ``distinct_x`` / ``distinct_y`` count the
    distinct distances.  All six are None when ranks were not asked for, and after :meth:`merge`: ranks of disjoint
    pair ranges do not combine.

    With ``kendall=True`` the call also keeps and sorts every pair on the GPU: ``kendall_tau`` is Kendall's tau-b of all
    n pairs (``scipy.stats.kendalltau``; NaN for a constant column, n < 2 or a NaN distance), computed from the exact
    integers ``concordant``, ``discordant``, ``ties_x``, ``ties_y`` and ``ties_xy`` (Python ints: sums of t (t - 1) / 2
    over the tie groups of x, of y and of both; concordant + discordant + ties_x + ties_y - ties_xy = n (n - 1) / 2), from
    which gamma, Somers' D or tau-a follow as well.  No p-value: pairs that share a leaf are not independent.  All six
    are None when Kendall's tau was not asked for, and after :meth:`merge`.
    """

    n_pairs: int
    n_leaves: Optional[int]
    mean_x: float
    mean_y: float
    var_x: float
    var_y: float
    cov: float
    pearson_r: float
    min_x: float
    max_x: float
    min_y: float
    max_y: float
    hist: Optional[np.ndarray]
    xedges: Optional[np.ndarray]
    yedges: Optional[np.ndarray]
    shift_x: float = 0.0
    shift_y: float = 0.0
    sx: float = 0.0
    sy: float = 0.0
    sxx: float = 0.0
    syy: float = 0.0
    sxy: float = 0.0
    spearman_r: Optional[float] = None
    rank_sxy: Optional[int] = None
    rank_sxx: Optional[int] = None
    rank_syy: Optional[int] = None
    distinct_x: Optional[int] = None
    distinct_y: Optional[int] = None
    kendall_tau: Optional[float] = None
    concordant: Optional[int] = None
    discordant: Optional[int] = None
    ties_x: Optional[int] = None
    ties_y: Optional[int] = None
    ties_xy: Optional[int] = None

    @classmethod
    def from_sums(cls, n, shift_x, shift_y, sx, sy, sxx, syy, sxy, min_x, max_x, min_y, max_y, hist=None, xedges=None,
                  yedges=None, n_leaves=None, ranks=None, kendall=None):
        """Derive the statistics from sums about a shift (st_pair_moments); ``ranks``: the library's ``_capi.RankSums`` of
        the same pairs, or None; ``kendall``: its ``_capi.KendallCounts``, or None."""
        n = int(n)
        nan = float("nan")
        if n == 0:
            mean_x = mean_y = var_x = var_y = cov = r = nan
            min_x = max_x = min_y = max_y = nan
        else:
            mean_x = shift_x + sx / n
            mean_y = shift_y + sy / n
            var_x = (sxx - sx * sx / n) / n
            var_y = (syy - sy * sy / n) / n
            cov = (sxy - sx * sy / n) / n
            var_x, var_y = max(var_x, 0.0), max(var_y, 0.0)      # (rounding of a constant column)
            r = cov / math.sqrt(var_x * var_y) if var_x > 0 and var_y > 0 else nan
            if not math.isnan(r):
                r = min(1.0, max(-1.0, r))
        return cls(n_pairs=n, n_leaves=n_leaves, mean_x=mean_x, mean_y=mean_y, var_x=var_x, var_y=var_y, cov=cov,
                   pearson_r=r, min_x=float(min_x), max_x=float(max_x), min_y=float(min_y), max_y=float(max_y), hist=hist,
                   xedges=xedges, yedges=yedges, shift_x=float(shift_x), shift_y=float(shift_y), sx=float(sx),
                   sy=float(sy), sxx=float(sxx), syy=float(syy), sxy=float(sxy), **rank_fields(ranks), **kendall_fields(kendall))

    @classmethod
    def from_moments(cls, m, hist=None, xedges=None, yedges=None, n_leaves=None, ranks=None, kendall=None):
        """From the library's ``_capi.PairMoments`` and, if given, its ``_capi.RankSums`` and ``_capi.KendallCounts``."""
        return cls.from_sums(m.n, m.shift_x, m.shift_y, m.sx, m.sy, m.sxx, m.syy, m.sxy, m.min_x, m.max_x, m.min_y,
                             m.max_y, hist, xedges, yedges, n_leaves, ranks, kendall)

    @classmethod
    def merge(cls, a: "DistanceComparison", b: "DistanceComparison") -> "DistanceComparison":
        """Combine results over disjoint pair ranges (Chan et al.'s pairwise update, written on the shifted sums): b's
        sums are moved to a's shift, d = b.shift - a.shift, sum(x - a.shift) = b.sx + n_b d_x,
        sum(x - a.shift)^2 = b.sxx + 2 d_x b.sx + n_b d_x^2 (b.sxx itself where that is infinite), and so on, then added.
        The class of an infinite cross product depends on the shift it was summed about and is not recovered.
        Histograms add when both have the same edges (otherwise ValueError).  The rank fields (``spearman_r``, ``rank_*``,
        ``distinct_*``) of the result are None: a value's rank depends on every pair of its call, so ranks of disjoint
        ranges do not combine.  The Kendall fields are None for the same reason."""
        if b.n_pairs == 0:
            return a if a.rank_sxy is None and a.discordant is None else replace(a, **rank_fields(None), **kendall_fields(None))
        if a.n_pairs == 0:
            return replace(b, n_leaves=a.n_leaves if a.n_leaves == b.n_leaves else None, **rank_fields(None), **kendall_fields(None))
        hist = None
        if a.hist is not None or b.hist is not None:
            if a.hist is None or b.hist is None or not (np.array_equal(a.xedges, b.xedges) and np.array_equal(a.yedges, b.yedges)):
                raise ValueError("cannot merge results with different histograms")
            hist = a.hist + b.hist
        dx, dy, nb = b.shift_x - a.shift_x, b.shift_y - a.shift_y, b.n_pairs
        sx = a.sx + b.sx + nb * dx
        sy = a.sy + b.sy + nb * dy
        # (an infinite value makes b's squares +inf about any shift: moved, they would be inf - inf = NaN)
        sxx = a.sxx + b.sxx if math.isinf(b.sxx) else a.sxx + b.sxx + 2.0 * dx * b.sx + nb * dx * dx
        syy = a.syy + b.syy if math.isinf(b.syy) else a.syy + b.syy + 2.0 * dy * b.sy + nb * dy * dy
        sxy = a.sxy + b.sxy + dx * b.sy + dy * b.sx + nb * dx * dy
        return cls.from_sums(a.n_pairs + nb, a.shift_x, a.shift_y, sx, sy, sxx, syy, sxy,
                             np.fmin(a.min_x, b.min_x), np.fmax(a.max_x, b.max_x), np.fmin(a.min_y, b.min_y),
                             np.fmax(a.max_y, b.max_y), hist, a.xedges if hist is not None else None,
                             a.yedges if hist is not None else None, a.n_leaves if a.n_leaves == b.n_leaves else None)


def spearman_from_sums(n, n_nan, sxy, sxx, syy):
    """Spearman's rs from the exact sums: sxy / sqrt(sxx syy) clipped to [-1, 1]; NaN when a column is constant
    (sxx or syy 0), n < 2, or a pair held a NaN (scipy's nan_policy="propagate").  One square root of the product
    (below 2^186 for n <= 2^31 - 1), not the product of two: sqrt(s * s) == s in binary floating point, so sxy == sxx == syy
    gives 1.0 and sxy == -sxx -1.0 exactly, which sqrt(s) * sqrt(s) misses by an ulp for some s."""
    if n < 2 or n_nan > 0 or sxx <= 0 or syy <= 0:
        return float("nan")
    return min(1.0, max(-1.0, float(sxy) / math.sqrt(float(sxx) * float(syy))))


def rank_fields(ranks):
    """The rank fields of a DistanceComparison from a ``_capi.RankSums`` (None: all None)."""
    if ranks is None:
        return dict(spearman_r=None, rank_sxy=None, rank_sxx=None, rank_syy=None, distinct_x=None, distinct_y=None)
    sxy, sxx, syy = ranks.sxy, ranks.sxx, ranks.syy
    return dict(spearman_r=spearman_from_sums(int(ranks.n), int(ranks.n_nan), sxy, sxx, syy), rank_sxy=sxy, rank_sxx=sxx,
                rank_syy=syy, distinct_x=int(ranks.distinct_x), distinct_y=int(ranks.distinct_y))


def kendall_from_counts(n, n_nan, concordant, discordant, ties_x, ties_y):
    """Kendall's tau-b from the exact counts: (concordant - discordant) / sqrt((n0 - ties_x)(n0 - ties_y)), n0 =
    n (n - 1) / 2, clipped to [-1, 1]; NaN when a factor is 0, n < 2, or a pair held a NaN (scipy's
    nan_policy="propagate").  The integer numerator and the two integer factors are converted to float, then one square
    root of the product is taken, as in spearman_from_sums: identical columns (numerator == both factors) give 1.0 and
    negated ones -1.0 exactly."""
    n0 = int(n) * (int(n) - 1) // 2
    fx, fy = n0 - int(ties_x), n0 - int(ties_y)
    if n < 2 or n_nan > 0 or fx <= 0 or fy <= 0:
        return float("nan")
    return min(1.0, max(-1.0, float(int(concordant) - int(discordant)) / math.sqrt(float(fx) * float(fy))))


def kendall_fields(counts):
    """The Kendall fields of a DistanceComparison from a ``_capi.KendallCounts`` (None: all None)."""
    if counts is None:
        return dict(kendall_tau=None, concordant=None, discordant=None, ties_x=None, ties_y=None, ties_xy=None)
    con, dis, tx, ty, txy = int(counts.concordant), int(counts.discordant), int(counts.ties_x), int(counts.ties_y), int(counts.ties_xy)
    return dict(kendall_tau=kendall_from_counts(int(counts.n), int(counts.n_nan), con, dis, tx, ty), concordant=con,
                discordant=dis, ties_x=tx, ties_y=ty, ties_xy=txy)


def histogram_edges(bins, range, min_max):
    """(xedges, yedges) exactly as numpy.histogram2d builds them for ``bins`` / ``range``.  With ``range=None`` the range of
    integer bins is the data's (min_x, max_x), (min_y, max_y), given as ``min_max`` (numpy widens an empty range by 0.5 on
    each side); edge arrays need neither."""
    if range is None and min_max is not None:
        range = [(min_max[0], min_max[1]), (min_max[2], min_max[3])]
    _, xedges, yedges = np.histogram2d(np.empty(0), np.empty(0), bins=bins, range=range)
    return np.ascontiguousarray(xedges, dtype=np.float64), np.ascontiguousarray(yedges, dtype=np.float64)


def _needs_data_range(bins, range):
    """True when numpy would take (part of) the range from the data: integer bins and no explicit range."""
    if range is not None:
        return False
    try:
        if len(bins) == 2:      # a pair: ints and / or edge arrays
            return any(np.ndim(b) == 0 for b in bins)
    except TypeError:
        return True             # one int for both axes
    return np.ndim(bins) == 0   # one edge array for both axes


def run(dx, dy, kind, arrays, bins, range, n_leaves=None, spearman=False, kendall=False):
    """The library calls behind compare_distances and linked_distances_summary, over one pair input of the
    ``_capi.DeviceTree`` s ``dx`` (x) and ``dy`` (y): ``kind`` "triangle" with ``arrays`` = two aligned id lists, or "pairs"
    with two (n, 2) id arrays.  ``kendall`` and ``spearman`` each cost their own call, in that order, which also returns
    the moments: without ``bins`` no other call is made.  With ``bins`` the moments call follows with the edges, after
    one without when ``range=None`` leaves numpy's range to the data (the first pass finds min and max, the second
    bins), and the moments are its.  With none of the three there is one moments call."""
    def call(stat, **kw):
        return getattr(dx, "compare_%s%s_host" % (kind, stat))(dy, *arrays, **kw)

    ranks = counts = hist = xedges = yedges = None
    if kendall:
        m, counts = call("_kendall")
    if spearman:
        m, ranks = call("_ranks")
    if bins is not None:
        if _needs_data_range(bins, range):
            m, _ = call("", edges=None)
            if m.n == 0:
                raise ValueError("autodetected range of an empty set of pairs: give range=")
            mm = (m.min_x, m.max_x, m.min_y, m.max_y)
            if not all(np.isfinite(mm)):
                raise ValueError("autodetected range of [%r, %r] x [%r, %r] is not finite" % mm)
            xedges, yedges = histogram_edges(bins, None, mm)
        else:
            xedges, yedges = histogram_edges(bins, range, None)
        m, hist = call("", edges=(xedges, yedges))
    elif not (spearman or kendall):
        m, _ = call("", edges=None)
    return DistanceComparison.from_moments(m, hist, xedges, yedges, n_leaves=n_leaves, ranks=ranks, kendall=counts)


def pearson_pvalue(r, n):
    """Two-sided p of ``scipy.stats.pearsonr`` for correlation ``r`` over ``n`` pairs, vectorised: 2 * betaincc(a, a,
    (|r| + 1) / 2) with a = n/2 - 1, 1.0 where n == 2 (NaN where r is), NaN where n < 2.  All NaN without scipy."""
    r = np.asarray(r, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    p = np.full(np.broadcast(r, n).shape, np.nan)
    try:
        from scipy import special
    except ImportError:
        return p
    big = (n > 2) & ~np.isnan(r)
    if big.any():
        ab = n[big] / 2 - 1
        p[big] = 2 * special.betaincc(ab, ab, (np.abs(np.clip(r[big], -1.0, 1.0)) + 1) / 2)
    p[(n == 2) & ~np.isnan(r)] = 1.0
    return p


_SUMS = ("shift_x", "shift_y", "sx", "sy", "sxx", "syy", "sxy")


def row_stats(n, shift_x, shift_y, sx, sy, sxx, syy, sxy):
    """(mean_x, mean_y, var_x, var_y, cov, pearson_r) of rows of sums: the formulas of DistanceComparison.from_sums,
    elementwise in the same order (the same bits as from_sums on each row)."""
    n = np.asarray(n).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_x = shift_x + sx / n
        mean_y = shift_y + sy / n
        var_x = np.maximum((sxx - sx * sx / n) / n, 0.0)
        var_y = np.maximum((syy - sy * sy / n) / n, 0.0)
        cov = (sxy - sx * sy / n) / n
        ok = (var_x > 0) & (var_y > 0)
        r = np.where(ok, np.clip(cov / np.sqrt(var_x * var_y), -1.0, 1.0), np.nan)
    return mean_x, mean_y, var_x, var_y, cov, r


class CladeComparisons:
    """One row per clade: the summary :meth:`SuchLinkedTrees.linked_distances_summary` gives after subsetting to that
    clade (SuchLinkedTrees.linked_distances_by_clade), as numpy columns.

    ``nodes`` are clade-tree node ids in ``get_internal_nodes()`` order; ``n_leaves`` the clade's leaf count
    (``subset_b_size`` / ``subset_a_size``), ``n_links`` its ``subset_n_links``, ``n_pairs`` = n_links (n_links - 1) / 2.
    x is always TreeA and y TreeB: ``mean_a`` / ``var_a`` / ``min_a`` / ``max_a`` describe the TreeA column,
    ``*_b`` the TreeB column, ``cov`` their population covariance, ``pearson_r`` Pearson's r (NaN where a variance is 0)
    and ``pvalue`` the two-sided p of ``scipy.stats.pearsonr`` (NaN when scipy is not installed).  The shifted raw sums
    ``shift_x`` ... ``sxy`` (x = TreeA) are kept, so :meth:`comparison` rebuilds any row as a DistanceComparison.
    """

    def __init__(self, nodes, n_leaves, n_links, sums, min_a, max_a, min_b, max_b, tree="B"):
        self.tree = tree
        self.nodes = np.asarray(nodes, dtype=np.int64)
        self.n_leaves = np.asarray(n_leaves, dtype=np.int64)
        self.n_links = np.asarray(n_links, dtype=np.int64)
        self.n_pairs = self.n_links * (self.n_links - 1) // 2
        for k in _SUMS:
            setattr(self, k, np.asarray(sums[k], dtype=np.float64))
        self.min_a, self.max_a = np.asarray(min_a, dtype=np.float64), np.asarray(max_a, dtype=np.float64)
        self.min_b, self.max_b = np.asarray(min_b, dtype=np.float64), np.asarray(max_b, dtype=np.float64)
        self.mean_a, self.mean_b, self.var_a, self.var_b, self.cov, self.pearson_r = row_stats(
            self.n_pairs, *(getattr(self, k) for k in _SUMS))
        self.pvalue = pearson_pvalue(self.pearson_r, self.n_pairs)
        self._row = None

    def __len__(self):
        return len(self.nodes)

    def comparison_at(self, i) -> DistanceComparison:
        """Row i as a DistanceComparison (``n_leaves`` = the row's link count, as linked_distances_summary reports)."""
        return DistanceComparison.from_sums(int(self.n_pairs[i]), *(float(getattr(self, k)[i]) for k in _SUMS),
                                            self.min_a[i], self.max_a[i], self.min_b[i], self.max_b[i],
                                            n_leaves=int(self.n_links[i]))

    def comparison(self, node) -> DistanceComparison:
        """The row of clade ``node`` as a DistanceComparison (KeyError for a node without a row)."""
        if self._row is None:
            self._row = {int(v): i for i, v in enumerate(self.nodes)}
        return self.comparison_at(self._row[int(node)])

    def to_dataframe(self):
        """The table of the per-clade notebook loop: ``name`` = "clade_<id>", ``n_links``, ``n_leafs``, ``r``, ``p``,
        then the other columns (pandas, imported here)."""
        import pandas as pd
        cols = {"name": ["clade_%d" % v for v in self.nodes], "n_links": self.n_links, "n_leafs": self.n_leaves,
                "r": self.pearson_r, "p": self.pvalue, "node": self.nodes, "n_pairs": self.n_pairs}
        for k in ("mean_a", "mean_b", "var_a", "var_b", "cov", "min_a", "max_a", "min_b", "max_b") + _SUMS:
            cols[k] = getattr(self, k)
        return pd.DataFrame(cols)


@dataclass(frozen=True)
class HommolaResult:
    """Hommola et al.'s (2009) permutation test of cospeciation (SuchLinkedTrees.hommola_cospeciation).

    ``corr_coeff`` is Pearson's r of the unpermuted links (x = TreeA, y = TreeB), ``observed`` their full summary,
    ``perm_stats`` the r of each permutation in draw order (float64, ``permutations`` of them) and ``p_value`` scikit-bio's
    (count(perm_stats >= corr_coeff) + 1) / (permutations + 1).  ``seed`` repeats the run.  Iterating gives
    ``(corr_coeff, p_value, perm_stats)``, as scikit-bio's ``hommola_cospeciation`` returns them.
    """

    corr_coeff: float
    p_value: float
    perm_stats: np.ndarray
    observed: DistanceComparison
    n_links: int
    permutations: int
    seed: int

    def __iter__(self):
        return iter((self.corr_coeff, self.p_value, self.perm_stats))


def hommola_pvalue(corr_coeff, perm_stats):
    """scikit-bio's rule: (number of permuted r >= the observed r, NaN not counted, + 1) / (permutations + 1); NaN when
    the observed r is NaN or there are no permutations."""
    perm_stats = np.asarray(perm_stats, dtype=np.float64)
    if math.isnan(corr_coeff) or perm_stats.size == 0:
        return float("nan")
    return (int(np.count_nonzero(perm_stats >= corr_coeff)) + 1) / (perm_stats.size + 1)


def hommola_rows(u_a, u_b, pos_a, pos_b, permutations, seed, batch):
    """The rows of Hommola's test as (ids_a, ids_b), C-order int64 (rows, n_links), in batches of at most ``batch`` rows.

    Link j is leaf ``u_a[pos_a[j]]`` of TreeA and ``u_b[pos_b[j]]`` of TreeB (``u_a`` / ``u_b``: the universes).  The
    first batch is row 0 alone, the links as they are.  Then permutation p = 1 .. ``permutations``, drawn in order from
    ``numpy.random.default_rng(seed)`` as scikit-bio's hommola_cospeciation draws them -- mp = rng.permutation(len(u_b)),
    then mh = rng.permutation(len(u_a)) -- relabels the links: ids_b = u_b[mp[pos_b]], ids_a = u_a[mh[pos_a]].  Draws
    happen as batches are taken, so the first k permutations are the same for any ``permutations`` >= k and any batch.
    Host memory is the batch's ids plus one permutation of each universe at a time."""
    u_a, u_b = np.asarray(u_a, dtype=np.int64), np.asarray(u_b, dtype=np.int64)
    pos_a, pos_b = np.asarray(pos_a, dtype=np.int64), np.asarray(pos_b, dtype=np.int64)
    yield u_a[pos_a][None, :], u_b[pos_b][None, :]
    rng = np.random.default_rng(seed)
    na, nb = len(u_a), len(u_b)
    done = 0
    while done < permutations:
        k = min(int(batch), permutations - done)
        ids_a = np.empty((k, len(pos_a)), dtype=np.int64)
        ids_b = np.empty((k, len(pos_b)), dtype=np.int64)
        for i in range(k):      # (only each draw's image is kept: memory grows with the links, not the universes)
            ids_b[i] = u_b[rng.permutation(nb)[pos_b]]
            ids_a[i] = u_a[rng.permutation(na)[pos_a]]
        done += k
        yield ids_a, ids_b


class CladeHommola:
    """Hommola's permutation test for every clade of one tree (SuchLinkedTrees.hommola_by_clade), as numpy columns.

    ``nodes`` are clade-tree node ids in ``get_internal_nodes()`` order; ``n_leaves`` the clade's leaf count, ``n_links``
    its links, ``n_pairs`` = n_links (n_links - 1) / 2.  ``corr_coeff`` is Pearson's r of the unpermuted links (x = TreeA,
    y = TreeB; the clade's ``pearson_r`` of linked_distances_by_clade), ``n_ge`` the number of permuted r >= it (NaN not
    counted), ``n_nan`` the permuted rows whose r is NaN and ``p_value`` = (n_ge + 1) / (permutations + 1), NaN where
    ``corr_coeff`` is.  ``perm_stats`` is the (rows,
    permutations) float64 array of permuted r with ``keep_stats=True``, else None.  ``permutations``, ``seed`` and
    ``tree`` repeat the call; ``skipped_nodes`` lists the clades of more than ``max_leaves`` leaves, which were not
    evaluated.
    """

    def __init__(self, nodes, n_leaves, n_links, observed, n_ge, n_nan, perm_stats, permutations, seed, tree, skipped_nodes):
        self.tree, self.permutations, self.seed = tree, int(permutations), int(seed)
        self.nodes = np.asarray(nodes, dtype=np.int64)
        self.n_leaves = np.asarray(n_leaves, dtype=np.int64)
        self.n_links = np.asarray(n_links, dtype=np.int64)
        self.n_pairs = self.n_links * (self.n_links - 1) // 2
        self._observed = observed      # st_pair_moments records of the unpermuted links, x = TreeA
        self.corr_coeff = row_stats(observed["n"], *(observed[k] for k in _SUMS))[5] if len(observed) else np.empty(0)
        self.n_ge = np.asarray(n_ge, dtype=np.int64)
        self.n_nan = np.asarray(n_nan, dtype=np.int64)
        self.p_value = np.where(np.isnan(self.corr_coeff), np.nan, (self.n_ge + 1) / (self.permutations + 1))
        self.perm_stats = perm_stats
        self.skipped_nodes = np.asarray(skipped_nodes, dtype=np.int64)
        self._row = None

    def __len__(self):
        return len(self.nodes)

    def result(self, node) -> "HommolaResult":
        """The row of clade ``node`` as a HommolaResult (KeyError for a node without a row): ``observed`` from the row's
        sums, ``perm_stats`` empty unless the call kept them."""
        if self._row is None:
            self._row = {int(v): i for i, v in enumerate(self.nodes)}
        i = self._row[int(node)]
        o = self._observed[i]
        observed = DistanceComparison.from_sums(int(o["n"]), *(float(o[k]) for k in _SUMS), float(o["min_x"]), float(o["max_x"]),
                                                float(o["min_y"]), float(o["max_y"]), n_leaves=int(self.n_links[i]))
        stats = self.perm_stats[i].copy() if self.perm_stats is not None else np.empty(0)
        return HommolaResult(float(self.corr_coeff[i]), float(self.p_value[i]), stats, observed, int(self.n_links[i]),
                             self.permutations, self.seed)

    def to_dataframe(self):
        """The table of the per-clade notebook loop: ``name`` = "clade_<id>", ``n_links``, ``n_leafs``, ``r``, ``p`` (the
        permutation p), then the other columns (pandas, imported here)."""
        import pandas as pd
        return pd.DataFrame({"name": ["clade_%d" % v for v in self.nodes], "n_links": self.n_links, "n_leafs": self.n_leaves,
                             "r": self.corr_coeff, "p": self.p_value, "node": self.nodes, "n_pairs": self.n_pairs,
                             "n_ge": self.n_ge, "n_nan": self.n_nan})


def hommola_permutation(seed, node, p, side, n, device=None):
    """The int32 permutation that SuchLinkedTrees.hommola_by_clade applies for (``seed``, clade ``node``, permutation
    index ``p`` >= 1, ``side``: 0 = the clade tree over the clade's own leaves, 1 = the other tree) over a universe of
    ``n`` leaves in depth-first order: a link at position i moves to position ``result[i]``; p = 0 is the identity.
    ``device=None`` computes it on the host, without a GPU; a device index runs the kernel's sort there -- the same
    values."""
    from . import _capi
    return _capi.hommola_permutation(seed, node, p, side, n, -1 if device is None else int(device))


def swap_null_tables(sets, n_universe, permutations=999, begin=0, iterations=None, seed=0, stream=0, device=None):
    """The degree-preserving swap null itself: randomised copies of a 0/1 matrix that keep its row sums and column sums
    (picante's ``independentswap`` / ``trialswap``), for any statistic of your own under the null of
    ``SuchTree.dispersion(null="swap")``.

    ``sets`` is an iterable of strictly increasing collections of positions 0 .. ``n_universe`` - 1 (3 to 16384): set r
    is row r, a position a column.  Returns ``(tables, offsets, accepted)``: ``tables[i]`` is draw p = ``begin`` + i, a
    uint16 array in which row r's columns, ascending, are ``tables[i, offsets[r]:offsets[r + 1]]``; p = 0 is the
    observation; ``accepted[i]`` the swaps chain p made of its ``iterations`` trials.  ``iterations=None`` is
    max(1000, 10 x the links), the library's own default (picante's is 1000 swaps).  Draw p depends on (seed, stream, p,
    iterations, the sets) alone.  ``device=None`` computes it on the host, without a GPU; a device index runs one
    wave per chain there -- the same values."""
    from . import _capi
    return _capi.swap_null_tables(sets, n_universe, permutations, begin, iterations, seed, stream, -1 if device is None else int(device))


class SetDispersion:
    """How closely related the members of each of many leaf sets are (SuchTree.dispersion,
    SuchLinkedTrees.partner_dispersion), as numpy columns, one entry per set.

    ``n`` is the set's size k, ``mpd`` the mean of the k (k - 1) ordered pairwise distances among its members and ``mntd``
    the mean over the members of the distance to the nearest other member (NaN for k < 2).  The null shuffles the labels
    of the universe (picante's ``null.model = "taxa.labels"``): under permutation p every set is relabelled by the same
    shuffle, so a set's null draws are uniform k-subsets of the universe, and the sets of a call share the shuffles.
    For ``x`` in (``mpd``, ``mntd``): ``x_null_mean`` and ``x_null_sd`` (the sample standard deviation, ddof = 1, as
    picante's ``sd``) over the null draws that are not NaN, ``x_ses`` = (x - mean) / sd -- NaN where the sd is 0 or
    undefined; NRI = -mpd_ses, NTI = -mntd_ses -- ``x_n_le`` the number of null draws <= x and ``x_p`` =
    (n_le + 1) / (permutations + 1), the lower tail: small when the members are clustered.  A null whose draws are all
    equal has sd 0 exactly; a set that is the whole universe has that null by definition (every draw is the set itself)
    and is reported so: mean = x, sd = 0, SES NaN, p = 1.  ``n_nan`` counts the null draws with a NaN in either statistic.
    ``null_mpd`` / ``null_mntd`` are the (sets, permutations) arrays of the draws with ``keep_null=True``, else None.
    ``permutations``, ``seed`` and ``n_universe`` repeat the call.  ``leaves`` / ``names`` are filled in by
    ``partner_dispersion``: the leaf whose partners a row describes.

    ``null`` is the null model, "taxa.labels" or "swap".  Under "swap" the draws are the rows of the call's 0/1 matrix
    after a chain of ``iterations`` trial swaps that keep both of its margins (``swap_null_tables``), and
    ``swap_accepted`` holds the swaps each chain made, entry p for null draw p (entry 0, the observation, is 0); under
    "taxa.labels" both are None.
    """

    COLUMNS = ("n", "mpd", "mntd", "mpd_null_mean", "mpd_null_sd", "mpd_ses", "mpd_n_le", "mpd_p", "mntd_null_mean", "mntd_null_sd",
               "mntd_ses", "mntd_n_le", "mntd_p", "n_nan")

    def __init__(self, n_sets, permutations, seed, n_universe, keep_null=False, null="taxa.labels", iterations=None):
        self.permutations, self.seed, self.n_universe = int(permutations), int(seed), int(n_universe)
        self.null, self.iterations = null, iterations
        self.swap_accepted = np.zeros(self.permutations + 1, dtype=np.int64) if null == "swap" else None
        self.n = np.zeros(n_sets, dtype=np.int64)
        for k in self.COLUMNS[1:]:
            setattr(self, k, np.zeros(n_sets, dtype=np.int64) if k.endswith("n_le") or k == "n_nan" else np.full(n_sets, np.nan))
        self.null_mpd = np.full((n_sets, self.permutations), np.nan) if keep_null else None
        self.null_mntd = np.full((n_sets, self.permutations), np.nan) if keep_null else None
        self.leaves = self.names = None

    def __len__(self):
        return len(self.n)

    def fill(self, at, k, records):
        """Reduce the (rows, permutations + 1) DISPERSION_RECORD array of sets [at, at + rows) of sizes ``k``."""
        k = np.asarray(k, dtype=np.int64)
        rows = slice(at, at + len(k))
        self.n[rows] = k
        kk = np.maximum(k, 2).astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            mpd = np.where(k[:, None] >= 2, records["pair_sum"] / (kk * (kk - 1)), np.nan)
            mntd = np.where(k[:, None] >= 2, records["nearest_sum"] / kk, np.nan)
        whole = k == self.n_universe
        self.n_nan[rows] = np.count_nonzero(np.isnan(mpd[:, 1:]) | np.isnan(mntd[:, 1:]), axis=1)
        for name, x in (("mpd", mpd), ("mntd", mntd)):
            mean, sd, ses, n_le = null_summary(x[:, 0], x[:, 1:], whole)
            getattr(self, name)[rows] = x[:, 0]
            getattr(self, name + "_null_mean")[rows] = mean
            getattr(self, name + "_null_sd")[rows] = sd
            getattr(self, name + "_ses")[rows] = ses
            getattr(self, name + "_n_le")[rows] = n_le
            getattr(self, name + "_p")[rows] = np.where(np.isnan(x[:, 0]), np.nan, (n_le + 1) / (self.permutations + 1))
            if self.null_mpd is not None:
                getattr(self, "null_" + name)[rows] = x[:, 1:]

    def row(self, i) -> dict:
        """Row i as a dict of Python scalars (plus ``leaf`` / ``name`` where the call knows them)."""
        out = {k: getattr(self, k)[i].item() for k in self.COLUMNS}
        if self.leaves is not None:
            out["leaf"], out["name"] = int(self.leaves[i]), self.names[i]
        return out

    def to_dataframe(self):
        """The columns as a pandas DataFrame (pandas imported here), ``leaf`` / ``name`` first where the call knows them."""
        import pandas as pd
        cols = {} if self.leaves is None else {"name": self.names, "leaf": self.leaves}
        cols.update({k: getattr(self, k) for k in self.COLUMNS})
        return pd.DataFrame(cols)


class SetUniFrac:
    """How different the members of every two of many leaf sets are, measured on the tree (SuchTree.unifrac,
    SuchLinkedTrees.partner_unifrac, unifrac_from_depths).

    ``n_sets`` sets; the pairs are ``[begin, begin + count)`` of the triangle k = i (i - 1) / 2 + j, 0 <= j < i < n_sets
    (:meth:`pair`).  ``pd_q`` (n_sets) and ``union_q`` (count) are exact int64 sums of depths in units of ``quantum`` =
    2^-``shift``: Faith's PD of every set -- the branch length that joins the root to its members -- and the same for
    the union of a pair's two sets.  They depend on (root, the sets, shift) alone, not on the range, the chunking or the
    device.  ``pd`` = ``pd_q`` * quantum (float64).  Condensed float64 arrays over the pairs: ``shared`` = PD_i + PD_j - U,
    the branch length both sets use; ``unifrac`` = (2 U - PD_i - PD_j) / U, the unweighted UniFrac distance (the share of
    the union's branch length that only one set uses); ``phylosor`` = 2 shared / (PD_i + PD_j); NaN where a denominator
    is 0.  ``leaves`` / ``names`` are filled in by ``partner_unifrac`` (the leaf whose partners a row describes), ``root``
    by the tree calls.
    """

    def __init__(self, n_sets, begin, shift, pd_q, union_q, root=None):
        self.n_sets, self.begin, self.shift = int(n_sets), int(begin), int(shift)
        self.pd_q = np.asarray(pd_q, dtype=np.int64)
        self.union_q = np.asarray(union_q, dtype=np.int64)
        self.count = len(self.union_q)
        self.quantum = math.ldexp(1.0, -self.shift)
        self.pd = self.pd_q.astype(np.float64) * self.quantum
        self.root = root
        self.leaves = self.names = None

    def __len__(self):
        return self.n_sets

    def pair(self, k):
        """(i, j), j < i, of pair ``k`` of this result (triangle index ``begin + k``)."""
        if not 0 <= k < self.count:
            raise IndexError("pair %d of %d" % (k, self.count))
        i, j = self._rows(np.array([self.begin + int(k)], dtype=np.int64))
        return int(i[0]), int(j[0])

    @staticmethod
    def _rows(k):
        i = ((1 + np.sqrt(1.0 + 8.0 * k.astype(np.float64))) // 2).astype(np.int64)
        i -= i * (i - 1) // 2 > k
        i += (i + 1) * i // 2 <= k
        return i, k - i * (i - 1) // 2

    def _sums(self):
        i, j = self._rows(self.begin + np.arange(self.count, dtype=np.int64))
        return self.pd_q[i] + self.pd_q[j]      # (exact: below 2^62)

    @property
    def shared(self):
        return (self._sums() - self.union_q).astype(np.float64) * self.quantum

    @property
    def unifrac(self):
        both = self._sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.union_q != 0, (2 * self.union_q - both) / self.union_q.astype(np.float64), np.nan)

    @property
    def phylosor(self):
        both = self._sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(both != 0, 2 * (both - self.union_q) / both.astype(np.float64), np.nan)

    def matrix(self, which="unifrac"):
        """The square symmetric (n_sets, n_sets) form of ``which`` ("unifrac", "phylosor" or "shared") with a zero
        diagonal; only where the result holds the whole triangle."""
        if which not in ("unifrac", "phylosor", "shared"):
            raise ValueError("which must be 'unifrac', 'phylosor' or 'shared'")
        if self.begin != 0 or self.count != self.n_sets * (self.n_sets - 1) // 2:
            raise ValueError("matrix() needs the whole triangle, this result holds pairs [%d, +%d)" % (self.begin, self.count))
        out = np.zeros((self.n_sets, self.n_sets))
        i, j = self._rows(np.arange(self.count, dtype=np.int64))
        out[i, j] = out[j, i] = getattr(self, which)
        return out

    def to_dataframe(self):
        """One row per pair as a pandas DataFrame (pandas imported here): i, j (and the two names where the call knows them),
        union, shared, unifrac, phylosor."""
        import pandas as pd
        i, j = self._rows(self.begin + np.arange(self.count, dtype=np.int64))
        cols = {"i": i, "j": j}
        if self.names is not None:
            cols["name_i"], cols["name_j"] = [self.names[v] for v in i], [self.names[v] for v in j]
        cols.update({"union": self.union_q.astype(np.float64) * self.quantum, "shared": self.shared, "unifrac": self.unifrac,
                     "phylosor": self.phylosor})
        return pd.DataFrame(cols)


class SetBetaDispersion:
    """How far apart the members of every two of many leaf sets are, by distance (SuchTree.beta_dispersion,
    SuchLinkedTrees.partner_beta_dispersion), as numpy columns, one entry per pair.

    ``n_sets`` sets; the pairs are ``[begin, begin + count)`` of the triangle k = i (i - 1) / 2 + j, 0 <= j < i < n_sets
    (:meth:`pair`).  ``n_i`` / ``n_j`` are the two sets' sizes and ``shared`` the number of members they have in common.
    ``beta_mpd`` is the mean distance between a member of one set and a member of the other, ``beta_mntd`` the mean, over
    the members of both sets, of the distance to the nearest member of the other set (picante's ``comdist`` /
    ``comdistnt``, unweighted); with ``exclude_shared`` a member is not compared with itself in the other set
    (``exclude.conspecifics``).  NaN where nothing is compared.  The null shuffles the labels of the universe, as in
    :class:`SetDispersion`, one shuffle serving every pair.  For ``x`` in (``beta_mpd``, ``beta_mntd``): ``x_null_mean``,
    ``x_null_sd`` (ddof = 1), ``x_ses`` = (x - mean) / sd -- betaNRI is ``beta_mpd_ses``, betaNTI ``beta_mntd_ses`` --
    ``x_n_le`` / ``x_n_ge`` the numbers of null draws <= x / >= x, and ``x_p_le`` = (n_le + 1) / (permutations + 1), ``x_p_ge``
    likewise: the two tails.  A pair of two sets that are both the whole universe has the observation as its null by
    definition and is reported so: mean = x, sd = 0, SES NaN, both p = 1.  ``n_nan`` counts the null draws with a NaN in
    either statistic.  ``null_beta_mpd`` / ``null_beta_mntd`` are the (pairs, permutations) draws with ``keep_null=True``,
    else None.  ``begin``, ``count``, ``permutations``, ``seed``, ``n_universe`` and ``exclude_shared`` repeat the call.
    ``leaves`` / ``names`` are filled in by ``partner_beta_dispersion``: the leaf whose partners set i is.
    """

    STATS = ("beta_mpd", "beta_mntd")
    COLUMNS = ("n_i", "n_j", "shared") + tuple(x + s for x in STATS for s in ("", "_null_mean", "_null_sd", "_ses", "_n_le", "_n_ge", "_p_le", "_p_ge")) \
        + ("n_nan",)

    def __init__(self, n_sets, begin, count, permutations, seed, n_universe, exclude_shared=False, keep_null=False):
        self.n_sets, self.begin, self.count = int(n_sets), int(begin), int(count)
        self.permutations, self.seed, self.n_universe = int(permutations), int(seed), int(n_universe)
        self.exclude_shared = bool(exclude_shared)
        for k in self.COLUMNS:
            whole = k in ("n_i", "n_j", "shared", "n_nan") or k.endswith("n_le") or k.endswith("n_ge")
            setattr(self, k, np.zeros(self.count, dtype=np.int64) if whole else np.full(self.count, np.nan))
        self.null_beta_mpd = np.full((self.count, self.permutations), np.nan) if keep_null else None
        self.null_beta_mntd = np.full((self.count, self.permutations), np.nan) if keep_null else None
        self.leaves = self.names = None

    def __len__(self):
        return self.count

    def pair(self, k):
        """(i, j), j < i, of pair ``k`` of this result (triangle index ``begin + k``)."""
        if not 0 <= k < self.count:
            raise IndexError("pair %d of %d" % (k, self.count))
        i, j = SetUniFrac._rows(np.array([self.begin + int(k)], dtype=np.int64))
        return int(i[0]), int(j[0])

    def fill(self, at, n_i, n_j, shared, records):
        """Reduce the (pairs, 2, permutations + 1) DISPERSION_RECORD array of pairs [at, at + pairs) of this result, whose
        sets have ``n_i`` and ``n_j`` members, ``shared`` of them in common."""
        n_i, n_j, shared = (np.asarray(v, dtype=np.int64) for v in (n_i, n_j, shared))
        rows = slice(at, at + len(n_i))
        self.n_i[rows], self.n_j[rows], self.shared[rows] = n_i, n_j, shared
        cross = records["pair_sum"][:, 0, :] + records["pair_sum"][:, 1, :]
        near = records["nearest_sum"][:, 0, :] + records["nearest_sum"][:, 1, :]
        left_out = shared if self.exclude_shared else np.zeros_like(shared)
        # members with nobody to be compared with: all of one set when the other is empty, the shared one when it is all the other has
        alone = self.exclude_shared & (shared == 1)
        z = np.where(n_j == 0, n_i, alone & (n_j == 1)) + np.where(n_i == 0, n_j, alone & (n_i == 1))
        den_mpd = (2 * (n_i * n_j - left_out)).astype(np.float64)[:, None]
        den_mntd = (n_i + n_j - z).astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            mpd = np.where(den_mpd > 0, cross / den_mpd, np.nan)
            mntd = np.where(den_mntd > 0, near / den_mntd, np.nan)
        whole = (n_i == self.n_universe) & (n_j == self.n_universe)
        self.n_nan[rows] = np.count_nonzero(np.isnan(mpd[:, 1:]) | np.isnan(mntd[:, 1:]), axis=1)
        for name, x in (("beta_mpd", mpd), ("beta_mntd", mntd)):
            mean, sd, ses, n_le = null_summary(x[:, 0], x[:, 1:], whole)
            n_ge = np.count_nonzero(x[:, 1:] >= x[:, :1], axis=1)
            if self.permutations:
                n_ge = np.where(whole & ~np.isnan(x[:, 0]), self.permutations, n_ge)
            getattr(self, name)[rows] = x[:, 0]
            for suffix, v in (("_null_mean", mean), ("_null_sd", sd), ("_ses", ses), ("_n_le", n_le), ("_n_ge", n_ge)):
                getattr(self, name + suffix)[rows] = v
            for tail, v in (("_p_le", n_le), ("_p_ge", n_ge)):
                getattr(self, name + tail)[rows] = np.where(np.isnan(x[:, 0]), np.nan, (v + 1) / (self.permutations + 1))
            if self.null_beta_mpd is not None:
                getattr(self, "null_" + name)[rows] = x[:, 1:]

    def matrix(self, which="beta_mntd"):
        """The square symmetric (n_sets, n_sets) form of a float column (``beta_mpd``, ``beta_mntd_ses``, ...) with a zero
        diagonal; only where the result holds the whole triangle."""
        if which not in self.COLUMNS or getattr(self, which).dtype != np.float64:
            raise ValueError("which must be one of the float columns, such as 'beta_mpd', 'beta_mntd' or 'beta_mntd_ses'")
        if self.begin != 0 or self.count != self.n_sets * (self.n_sets - 1) // 2:
            raise ValueError("matrix() needs the whole triangle, this result holds pairs [%d, +%d)" % (self.begin, self.count))
        out = np.zeros((self.n_sets, self.n_sets))
        i, j = SetUniFrac._rows(np.arange(self.count, dtype=np.int64))
        out[i, j] = out[j, i] = getattr(self, which)
        return out

    def row(self, k) -> dict:
        """Pair k as a dict of Python scalars: ``i``, ``j`` (and the two names where the call knows them), then the columns."""
        i, j = self.pair(k)
        out = {"i": i, "j": j}
        if self.names is not None:
            out["name_i"], out["name_j"] = self.names[i], self.names[j]
        out.update({c: getattr(self, c)[k].item() for c in self.COLUMNS})
        return out

    def to_dataframe(self):
        """One row per pair as a pandas DataFrame (pandas imported here): i, j (and the two names where the call knows
        them), then the columns."""
        import pandas as pd
        i, j = SetUniFrac._rows(self.begin + np.arange(self.count, dtype=np.int64))
        cols = {"i": i, "j": j}
        if self.names is not None:
            cols["name_i"], cols["name_j"] = [self.names[v] for v in i], [self.names[v] for v in j]
        cols.update({c: getattr(self, c) for c in self.COLUMNS})
        return pd.DataFrame(cols)


class SetUniFracNull:
    """Faith's PD of many leaf sets and the UniFrac and PhyloSor of their pairs, each standardised against the null that
    shuffles the universe's leaf labels (SuchTree.unifrac_null, SuchLinkedTrees.partner_unifrac_null): picante's ``ses.pd``
    with ``null.model = "taxa.labels"``, and the label-shuffling significance of UniFrac (Lozupone & Knight 2005).

    ``n_sets`` sets; the pairs are ``[begin, begin + count)`` of the triangle k = i (i - 1) / 2 + j, 0 <= j < i < n_sets
    (:meth:`pair`).  Under permutation p every set is relabelled by the same shuffle, as in :class:`SetDispersion`, and
    every sum is taken again: exact int64 sums in units of ``quantum`` = 2^-``shift``, as in :class:`SetUniFrac`.

    Per set: ``n`` its size, ``pd_q`` the observed integer sum, ``pd`` = ``pd_q`` * quantum, ``pd_null_mean``,
    ``pd_null_sd`` (ddof = 1), ``pd_ses`` = (pd - mean) / sd (NaN where the sd is 0 or undefined), ``pd_n_le`` /
    ``pd_n_ge`` the numbers of null draws <= / >= the observation and ``pd_p_le`` = (n_le + 1) / (permutations + 1),
    ``pd_p_ge`` likewise: the two tails.  Per pair: ``union_q`` and, for ``x`` in (``unifrac``, ``phylosor``) -- formed
    from the integers of a draw by the expressions of :class:`SetUniFrac`, NaN where a denominator is 0 -- ``x`` and the
    same eight null columns; ``n_nan`` counts the pair's null draws with a NaN in either statistic.  A set that is the
    whole universe has the observation as its null by definition and is reported so: mean = x, sd = 0, SES NaN, both
    p = 1; the same holds for a pair of two such sets.  With ``keep_null=True`` ``null_pd`` is the (sets, permutations)
    array of draws and ``null_unifrac`` / ``null_phylosor`` the (pairs, permutations) ones, else None.  ``permutations``,
    ``seed``, ``n_universe``, ``shift``, ``begin`` and ``count`` repeat the call; ``leaves`` / ``names`` are filled in by
    ``partner_unifrac_null`` (the leaf whose partners a set is), ``root`` by the tree calls.
    """

    STATS = ("unifrac", "phylosor")
    SET_COLUMNS = ("n", "pd_q", "pd", "pd_null_mean", "pd_null_sd", "pd_ses", "pd_n_le", "pd_n_ge", "pd_p_le", "pd_p_ge")
    COLUMNS = ("union_q",) + tuple(x + s for x in STATS for s in ("", "_null_mean", "_null_sd", "_ses", "_n_le", "_n_ge", "_p_le", "_p_ge")) \
        + ("n_nan",)

    def __init__(self, n_sets, begin, count, shift, permutations, seed, n_universe, keep_null=False, root=None):
        self.n_sets, self.begin, self.count, self.shift = int(n_sets), int(begin), int(count), int(shift)
        self.permutations, self.seed, self.n_universe = int(permutations), int(seed), int(n_universe)
        self.quantum = math.ldexp(1.0, -self.shift)
        for cols, rows in ((self.SET_COLUMNS, self.n_sets), (self.COLUMNS, self.count)):
            for k in cols:
                whole = k in ("n", "pd_q", "union_q", "n_nan") or k.endswith("n_le") or k.endswith("n_ge")
                setattr(self, k, np.zeros(rows, dtype=np.int64) if whole else np.full(rows, np.nan))
        self.null_pd = np.full((self.n_sets, self.permutations), np.nan) if keep_null else None
        self.null_unifrac = np.full((self.count, self.permutations), np.nan) if keep_null else None
        self.null_phylosor = np.full((self.count, self.permutations), np.nan) if keep_null else None
        self._pd_block = np.zeros((self.n_sets, self.permutations + 1), dtype=np.int64)
        self.root = root
        self.leaves = self.names = None

    def __len__(self):
        return self.n_sets

    def pair(self, k):
        """(i, j), j < i, of pair ``k`` of this result (triangle index ``begin + k``)."""
        if not 0 <= k < self.count:
            raise IndexError("pair %d of %d" % (k, self.count))
        i, j = SetUniFrac._rows(np.array([self.begin + int(k)], dtype=np.int64))
        return int(i[0]), int(j[0])

    def _reduce(self, name, rows, x, whole):
        """The eight null columns of statistic ``name`` over ``rows`` from x (rows, permutations + 1), column 0 observed."""
        mean, sd, ses, n_le = null_summary(x[:, 0], x[:, 1:], whole)
        n_ge = np.count_nonzero(x[:, 1:] >= x[:, :1], axis=1)
        if self.permutations:
            n_ge = np.where(whole & ~np.isnan(x[:, 0]), self.permutations, n_ge)
        getattr(self, name)[rows] = x[:, 0]
        for suffix, v in (("_null_mean", mean), ("_null_sd", sd), ("_ses", ses), ("_n_le", n_le), ("_n_ge", n_ge)):
            getattr(self, name + suffix)[rows] = v
        for tail, v in (("_p_le", n_le), ("_p_ge", n_ge)):
            getattr(self, name + tail)[rows] = np.where(np.isnan(x[:, 0]), np.nan, (v + 1) / (self.permutations + 1))
        if self.null_pd is not None:
            getattr(self, "null_" + name)[rows] = x[:, 1:]

    def fill_sets(self, k, pd_block):
        """Reduce the (n_sets, permutations + 1) int64 block of PD sums of the sets, of sizes ``k``; before any fill_pairs."""
        self.n[:] = np.asarray(k, dtype=np.int64)
        self._pd_block[:] = pd_block
        self.pd_q[:] = self._pd_block[:, 0]
        self._reduce("pd", slice(0, self.n_sets), self._pd_block.astype(np.float64) * self.quantum, self.n == self.n_universe)

    def fill_pairs(self, at, union_block):
        """Reduce the (pairs, permutations + 1) int64 block of union sums of pairs [at, at + pairs) of this result."""
        union = np.asarray(union_block, dtype=np.int64)
        rows = slice(at, at + len(union))
        i, j = SetUniFrac._rows(self.begin + at + np.arange(len(union), dtype=np.int64))
        both = self._pd_block[i] + self._pd_block[j]      # (exact: below 2^62)
        self.union_q[rows] = union[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            unifrac = np.where(union != 0, (2 * union - both) / union.astype(np.float64), np.nan)
            phylosor = np.where(both != 0, 2 * (both - union) / both.astype(np.float64), np.nan)
        whole = (self.n[i] == self.n_universe) & (self.n[j] == self.n_universe)
        self.n_nan[rows] = np.count_nonzero(np.isnan(unifrac[:, 1:]) | np.isnan(phylosor[:, 1:]), axis=1)
        self._reduce("unifrac", rows, unifrac, whole)
        self._reduce("phylosor", rows, phylosor, whole)

    def matrix(self, which="unifrac_ses"):
        """The square symmetric (n_sets, n_sets) form of a float pair column (``unifrac``, ``unifrac_ses``, ``phylosor_p_le``,
        ...) with a zero diagonal; only where the result holds the whole triangle."""
        if which not in self.COLUMNS or getattr(self, which).dtype != np.float64:
            raise ValueError("which must be one of the float pair columns, such as 'unifrac', 'unifrac_ses' or 'phylosor_ses'")
        if self.begin != 0 or self.count != self.n_sets * (self.n_sets - 1) // 2:
            raise ValueError("matrix() needs the whole triangle, this result holds pairs [%d, +%d)" % (self.begin, self.count))
        out = np.zeros((self.n_sets, self.n_sets))
        i, j = SetUniFrac._rows(np.arange(self.count, dtype=np.int64))
        out[i, j] = out[j, i] = getattr(self, which)
        return out

    def set_row(self, r) -> dict:
        """Set r as a dict of Python scalars (plus ``leaf`` / ``name`` where the call knows them)."""
        out = {c: getattr(self, c)[r].item() for c in self.SET_COLUMNS}
        if self.leaves is not None:
            out["leaf"], out["name"] = int(self.leaves[r]), self.names[r]
        return out

    def row(self, k) -> dict:
        """Pair k as a dict of Python scalars: ``i``, ``j`` (and the two names where the call knows them), then the columns."""
        i, j = self.pair(k)
        out = {"i": i, "j": j}
        if self.names is not None:
            out["name_i"], out["name_j"] = self.names[i], self.names[j]
        out.update({c: getattr(self, c)[k].item() for c in self.COLUMNS})
        return out

    def to_dataframe(self, which="pairs"):
        """A pandas DataFrame (pandas imported here): ``which="pairs"``, one row per pair -- i, j (and the two names where
        the call knows them), then the pair columns; ``which="sets"``, one row per set with the PD columns."""
        import pandas as pd
        if which == "sets":
            cols = {} if self.leaves is None else {"name": self.names, "leaf": self.leaves}
            cols.update({c: getattr(self, c) for c in self.SET_COLUMNS})
            return pd.DataFrame(cols)
        if which != "pairs":
            raise ValueError("which must be 'pairs' or 'sets'")
        i, j = SetUniFrac._rows(self.begin + np.arange(self.count, dtype=np.int64))
        cols = {"i": i, "j": j}
        if self.names is not None:
            cols["name_i"], cols["name_j"] = [self.names[v] for v in i], [self.names[v] for v in j]
        cols.update({c: getattr(self, c) for c in self.COLUMNS})
        return pd.DataFrame(cols)


def set_bit_rows(set_pos, offsets, n_universe):
    """The position sets (set_pos, offsets) over a universe of ``n_universe`` as rows of bits (uint8, eight positions each)."""
    n_sets = len(offsets) - 1
    bits = np.zeros((n_sets, (int(n_universe) + 7) // 8 * 8), dtype=bool)
    bits[np.repeat(np.arange(n_sets), np.diff(offsets)), set_pos] = True
    return np.packbits(bits, axis=1)


def shared_counts(bit_rows, i, j):
    """|S_i and S_j| for the pairs (i[k], j[k]) of the sets of ``set_bit_rows``: the rows ANDed a block of pairs at a time."""
    ones = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)
    out = np.zeros(len(i), dtype=np.int64)
    step = max(1, (1 << 24) // max(bit_rows.shape[1], 1))
    for at in range(0, len(i), step):
        out[at:at + step] = ones[bit_rows[i[at:at + step]] & bit_rows[j[at:at + step]]].sum(axis=1)
    return out


def unifrac_from_depths(d, h, sets, begin=0, count=None, shift=None, device=None, chunk_pairs=0):
    """:class:`SetUniFrac` of the position sets ``sets`` over a universe given by its float32 depths: ``d[k]`` the root
    distance of leaf k (leaves in depth-first order), ``h[k]`` that of the MRCA of leaves k and k + 1.  The depths are
    quantised by the rule of ``SuchTree.unifrac`` (``shift`` None = automatic).  ``device=None`` computes on the host,
    without a GPU; a device index runs the kernels there -- the same integers."""
    from . import _capi
    d_q, h_q, used = _capi.unifrac_quantise(d, h, shift)
    pd_q, union_q = _capi.unifrac_depths(d_q, h_q, sets, begin, count, -1 if device is None else int(device), chunk_pairs)
    return SetUniFrac(len(pd_q), begin, used, pd_q, union_q)


def clade_side(flat, leaf_ids, rooted=False, min_branch=None):
    """(order, node, lo, hi) of one tree over the listed leaves (``_capi.clade_ranges``): the depth-first order and the
    eligible induced clades, without those whose branch is ``min_branch`` or shorter.  A clade's branch is the path from
    its node up to the next node that is the MRCA of a larger set of listed leaves, summed in float64."""
    from . import _capi
    leaf_ids = np.ascontiguousarray(leaf_ids, dtype=np.int64)
    order, node, lo, hi = _capi.clade_ranges(flat.parent, leaf_ids, rooted)
    if min_branch is None or not len(node):
        return order, node, lo, hi
    parent, length = np.asarray(flat.parent), np.asarray(flat.distance, dtype=np.float64)
    stop = np.zeros(len(parent), dtype=bool)      # every kept node: the eligible ones of a rooted list, and the MRCA of all
    stop[_capi.clade_ranges(flat.parent, leaf_ids, True)[1]] = True
    above, v = set(), int(leaf_ids[order[0]])
    while v != -1:
        above.add(v)
        v = int(parent[v])
    v = int(leaf_ids[order[-1]])      # (the first and the last leaf in depth-first order meet at the MRCA of all)
    while v not in above:
        v = int(parent[v])
    stop[v] = True
    branch = np.zeros(len(node), dtype=np.float64)
    for r, v in enumerate(node):
        total, u = length[v], int(parent[v])
        while u != -1 and not stop[u]:
            total += length[u]
            u = int(parent[u])
        branch[r] = total
    keep = branch > float(min_branch)
    return order, node[keep], lo[keep], hi[keep]


class CladeMatches:
    """Every induced clade of tree A matched to the closest induced clade of tree B over m shared leaves
    (SuchTree.compare_clades).

    One row per clade of A, in ``get_internal_nodes()`` order: ``nodes`` (A node ids), ``n_leaves`` (listed leaves under
    the node), ``match`` (the B node id of the closest clade, the first in B's order on a tie; -1 where B has none),
    ``match_leaves`` and ``intersection`` (its size and the leaves the two share, 0 without a match), ``distance`` (delta:
    the leaves to move, d = n_leaves + match_leaves - 2 intersection, or min(d, m - d) when unrooted; -1 without a match),
    ``transfer`` = min(distance, p - 1) with p = n_leaves (rooted) or min(n_leaves, m - n_leaves) (unrooted), the
    transfer distance of Lemoine et al. 2018 (p - 1 without a match), ``support`` = 1 - transfer / (p - 1) and ``jaccard``
    = intersection / (n_leaves + match_leaves - intersection) of the two leaf sets as they stand (NaN without a match).
    Scalars over ALL clades of A, whatever ``nodes=`` kept as rows: ``n_a``, ``n_b`` (clades of either tree), ``exact``
    (clades of A with distance 0), ``rf`` = n_a + n_b - 2 exact (Robinson-Foulds), ``rf_normalised`` = rf / (n_a + n_b)
    (NaN when both are 0), ``mean_transfer``; ``n_leaves_shared`` = m and ``rooted`` repeat the call.  All columns but the
    last two are integers that do not depend on the device or the chunking.
    """

    COLUMNS = ("nodes", "n_leaves", "match", "match_leaves", "intersection", "distance", "transfer", "support", "jaccard")

    def __init__(self, m, rooted, side_a, side_b, distance, match, intersection, rows=None):
        _, node_a, lo_a, hi_a = side_a
        _, node_b, lo_b, hi_b = side_b
        self.n_leaves_shared, self.rooted = int(m), bool(rooted)
        self.n_a, self.n_b = len(node_a), len(node_b)
        size_a = (hi_a - lo_a).astype(np.int64)
        size_b = (hi_b - lo_b).astype(np.int64)
        distance, match = np.asarray(distance, dtype=np.int64), np.asarray(match, dtype=np.int64)
        found = match >= 0
        p = size_a if rooted else np.minimum(size_a, m - size_a)
        transfer = np.where(found, np.minimum(distance, p - 1), p - 1)
        self.exact = int((found & (distance == 0)).sum())
        self.rf = self.n_a + self.n_b - 2 * self.exact
        self.rf_normalised = self.rf / (self.n_a + self.n_b) if self.n_a + self.n_b else float("nan")
        self.mean_transfer = float(transfer.mean()) if self.n_a else float("nan")
        rows = np.arange(self.n_a) if rows is None else np.asarray(rows, dtype=np.int64)
        safe = np.where(found, match, 0)[rows]
        found = found[rows]
        self.nodes = node_a[rows].astype(np.int64)
        self.n_leaves = size_a[rows]
        self.match = np.where(found, node_b[safe] if self.n_b else -1, -1).astype(np.int64)
        self.match_leaves = np.where(found, size_b[safe] if self.n_b else 0, 0).astype(np.int64)
        self.intersection = np.where(found, np.asarray(intersection, dtype=np.int64)[rows], 0)
        self.distance = distance[rows]
        self.transfer = transfer[rows]
        self.support = 1.0 - self.transfer / (p[rows] - 1.0)
        union = self.n_leaves + self.match_leaves - self.intersection
        self.jaccard = np.where(found, self.intersection / union.astype(np.float64), np.nan)

    def __len__(self):
        return len(self.nodes)

    def row(self, node) -> dict:
        """The row of A's clade ``node`` as a dict of Python scalars (KeyError when it is not a row)."""
        at = np.flatnonzero(self.nodes == int(node))
        if not len(at):
            raise KeyError("node %r is not a row of this result" % (node,))
        return {("node" if k == "nodes" else k): getattr(self, k)[at[0]].item() for k in self.COLUMNS}

    def to_dataframe(self):
        """The columns as a pandas DataFrame (pandas imported here)."""
        import pandas as pd
        return pd.DataFrame({k: getattr(self, k) for k in self.COLUMNS})


def match_clades(flat_a, ids_a, flat_b, ids_b, rooted=False, nodes=None, min_branch=None, device=None, chunk_rows=0, side_a=None):
    """:class:`CladeMatches` of two flat trees over aligned leaf-id lists (leaf k is ``ids_a[k]`` in A and ``ids_b[k]`` in
    B).  ``device=None`` computes on the host, without a GPU; a device index runs the kernel there -- the same integers.
    ``side_a``: A's :func:`clade_side`, where the caller has it already (transfer_support, one A against many B)."""
    from . import _capi
    ids_a, ids_b = (np.ascontiguousarray(v, dtype=np.int64) for v in (ids_a, ids_b))
    if ids_a.ndim != 1 or ids_a.shape != ids_b.shape:
        raise ValueError("the two id lists must be 1-D and of equal length")
    m = len(ids_a)
    if m < 4 or m > _capi.CLADE_MATCH_MAX_LEAVES:
        raise ValueError("%d shared leaves: 4 to %d" % (m, _capi.CLADE_MATCH_MAX_LEAVES))
    if side_a is None:
        side_a = clade_side(flat_a, ids_a, rooted, min_branch)
    side_b = clade_side(flat_b, ids_b, rooted, min_branch)
    rows = None
    if nodes is not None:
        wanted = np.atleast_1d(np.asarray(nodes, dtype=np.int64))
        at = {int(v): r for r, v in enumerate(side_a[1])}
        for v in wanted:
            if int(v) not in at:
                raise ValueError("node %d is not a clade of this comparison" % v)
        rows = np.array([at[int(v)] for v in wanted], dtype=np.int64)
    where_b = np.empty(m, dtype=np.int32)
    where_b[side_b[0]] = np.arange(m, dtype=np.int32)
    got = _capi.clade_match(m, where_b[side_a[0]], side_a[2], side_a[3], side_b[2], side_b[3], rooted, -1 if device is None else int(device),
                            chunk_rows)
    return CladeMatches(m, rooted, side_a, side_b, *got, rows=rows)


class TransferSupport:
    """The transfer bootstrap expectation of every clade of a tree over replicate trees (SuchTree.transfer_support).

    One row per clade, in ``get_internal_nodes()`` order: ``nodes``, ``n_leaves``, ``transfer_sum`` (the exact int64 sum of
    the clade's transfer distance over the replicates), ``support`` = 1 - (transfer_sum / n_replicates) / (p - 1), the mean
    of the per-replicate supports (NaN without replicates), and ``exact_count``, the replicates that hold the clade itself:
    Felsenstein's bootstrap count.  ``n_replicates``, ``n_leaves_shared`` and ``rooted`` repeat the call.
    """

    COLUMNS = ("nodes", "n_leaves", "transfer_sum", "support", "exact_count")

    def __init__(self, m, rooted, side_a):
        _, node, lo, hi = side_a
        self.n_leaves_shared, self.rooted, self.n_replicates = int(m), bool(rooted), 0
        self.nodes = node.astype(np.int64)
        self.n_leaves = (hi - lo).astype(np.int64)
        self.transfer_sum = np.zeros(len(node), dtype=np.int64)
        self.exact_count = np.zeros(len(node), dtype=np.int64)

    def add(self, matches: CladeMatches):
        self.transfer_sum += matches.transfer
        self.exact_count += (matches.match >= 0) & (matches.distance == 0)
        self.n_replicates += 1

    @property
    def support(self):
        p = self.n_leaves if self.rooted else np.minimum(self.n_leaves, self.n_leaves_shared - self.n_leaves)
        if not self.n_replicates:
            return np.full(len(self.nodes), np.nan)
        return 1.0 - (self.transfer_sum / float(self.n_replicates)) / (p - 1.0)

    def __len__(self):
        return len(self.nodes)

    def row(self, node) -> dict:
        at = np.flatnonzero(self.nodes == int(node))
        if not len(at):
            raise KeyError("node %r is not a row of this result" % (node,))
        return {("node" if k == "nodes" else k): getattr(self, k)[at[0]].item() for k in self.COLUMNS}

    def to_dataframe(self):
        import pandas as pd
        return pd.DataFrame({k: getattr(self, k) for k in self.COLUMNS})


def read_flat_tree(tree, extended=False):
    """The flat arrays of one tree of a collection (transfer_support's replicates, :func:`tree_set`'s trees): a SuchTree's
    own, a Newick text or the path of a Newick file parsed to flat arrays only -- nothing goes to a GPU.  ``extended``
    also takes a :class:`Dendrogram` (through ``to_flat()``) and a flat tree itself.  None for anything else."""
    from .newick import flat_tree_from_newick
    from .suchtree import SuchTree
    if isinstance(tree, SuchTree):
        return tree._flat
    if isinstance(tree, str):
        text = tree.strip()
        if not (text.startswith("(") and text.endswith(";")):
            with open(tree) as fh:
                text = fh.read()
        return flat_tree_from_newick(text)
    if extended and isinstance(tree, Dendrogram):
        return tree.to_flat()
    if extended and all(hasattr(tree, k) for k in ("parent", "distance", "leaves")):
        return tree
    return None


# compare.tree_set(device=...) and compare.rf_relabelled(device=...) run the host restatement while tasks x leaves is
# below this and the kernel on device 0 from it on.  A device call costs 0.8 ms at 64 leaves to 2.6 ms at 16384 whatever it
# computes (the work block, the stream, the read-back ring), the host restatement about 0.02 to 0.06 microseconds per
# task and leaf.  Measured (profiles/tree_set_r33.log; medians of 5, beyond both spreads): the host wins up to 496 tasks
# of 64 leaves, 28 of 1024 and 1 of 16384 (31,744 / 28,672 / 16,384 tasks x leaves); the device wins from 1128 tasks of 64
# leaves, 66 of 1024 and 3 of 16384 (72,192 / 67,584 / 49,152).  72 x 1024 is at or above the first point the device won
# at in every column (README, "A whole set of trees")
RF_DEVICE_MIN_WORK = 73728


def _rf_device(device, n_tasks, m):
    """The ``device`` of _capi.rf_tasks for the ``device`` of a caller: ... follows RF_DEVICE_MIN_WORK."""
    from .suchtree import int_arg
    if device is ...:
        return 0 if n_tasks * m >= RF_DEVICE_MIN_WORK else -1
    return -1 if device is None else int_arg("device", device)


def _rf_sides(sides, m):
    """(where, offsets, lo, hi) of st_rf_tasks from one :func:`clade_side` per tree"""
    where = np.empty((len(sides), m), dtype=np.int32)
    for t, side in enumerate(sides):
        where[t, side[0]] = np.arange(m, dtype=np.int32)
    offsets = np.zeros(len(sides) + 1, dtype=np.int64)
    np.cumsum([len(side[1]) for side in sides], out=offsets[1:])
    cat = lambda k: np.concatenate([side[k] for side in sides]).astype(np.int32) if sides else np.zeros(0, dtype=np.int32)      # noqa: E731
    return where, offsets, cat(2), cat(3)


class TreeSetComparison:
    """Every two trees of a set compared by the clades they share (:func:`tree_set`).

    ``n_trees``, ``n_leaves_shared`` (m), ``rooted``, and the range ``begin`` / ``count`` of the triangle of pairs in the
    order k = i (i - 1) / 2 + j, j < i.  ``n_clades`` (int64, per tree) are the eligible clades.  Per pair of the range,
    condensed: ``shared`` (int64, the clades the two trees have in common), ``rf`` = n_i + n_j - 2 shared (int64, the
    Robinson-Foulds distance) and ``rf_normalised`` = rf / (n_i + n_j) (NaN where neither tree has a clade).  All
    integers: they do not depend on the device or the chunking.  ``leaves`` are the common leaf names, ``names`` one label
    per tree (its index, unless the caller set others).
    """

    COLUMNS = ("i", "j", "shared", "rf", "rf_normalised")

    def __init__(self, sides, m, rooted, begin, shared, counts, leaves):
        self.n_trees, self.n_leaves_shared, self.rooted = len(sides), int(m), bool(rooted)
        self.begin, self.count = int(begin), len(shared)
        self.n_clades = np.array([len(side[1]) for side in sides], dtype=np.int64)
        self.leaves, self.names = list(leaves), [str(t) for t in range(len(sides))]
        self._sides = sides
        k = np.arange(self.begin, self.begin + self.count, dtype=np.int64)
        i = ((1 + np.sqrt(8.0 * k + 1.0)) // 2).astype(np.int64)
        i = np.where(i * (i - 1) // 2 > k, i - 1, i)
        i = np.where((i + 1) * i // 2 <= k, i + 1, i)
        self.i, self.j = i, k - i * (i - 1) // 2
        self.shared = np.asarray(shared, dtype=np.int64)
        total = self.n_clades[self.i] + self.n_clades[self.j]
        self.rf = total - 2 * self.shared
        with np.errstate(invalid="ignore", divide="ignore"):
            self.rf_normalised = np.where(total > 0, self.rf / total.astype(np.float64), np.nan)
        self._frequency = None
        if counts is not None:
            offsets = np.concatenate([[0], np.cumsum(self.n_clades)])
            self._frequency = [np.asarray(counts[offsets[t]:offsets[t + 1]], dtype=np.int64) + 1 for t in range(self.n_trees)]

    def __len__(self):
        return self.count

    def __repr__(self):
        return "TreeSetComparison(n_trees=%d, n_leaves_shared=%d, rooted=%r, begin=%d, count=%d)" % (
            self.n_trees, self.n_leaves_shared, self.rooted, self.begin, self.count)

    def pair(self, k):
        """(i, j), j < i, of pair ``k`` of the range."""
        k = int(k)
        if not 0 <= k < self.count:
            raise IndexError("pair %d of %d" % (k, self.count))
        return int(self.i[k]), int(self.j[k])

    def matrix(self, which="rf"):
        """The square symmetric matrix of ``rf``, ``rf_normalised`` or ``shared`` with a zero diagonal: the whole triangle only."""
        if which not in ("rf", "rf_normalised", "shared"):
            raise ValueError("which must be 'rf', 'rf_normalised' or 'shared'")
        if self.begin != 0 or self.count != self.n_trees * (self.n_trees - 1) // 2:
            raise ValueError("a matrix needs the whole triangle, this result holds pairs [%d, %d)" % (self.begin, self.begin + self.count))
        v = getattr(self, which)
        M = np.zeros((self.n_trees, self.n_trees), dtype=v.dtype)
        M[self.i, self.j] = M[self.j, self.i] = v
        return M

    def clades(self, t):
        """(``nodes``, ``n_leaves``, ``frequency``) of tree ``t``'s eligible clades in ``get_internal_nodes()`` order:
        ``frequency`` (int64) is the number of trees of the set that hold the clade, the tree itself included -- None
        unless the call had ``frequencies=True`` and the whole triangle."""
        t = int(t)
        if not 0 <= t < self.n_trees:
            raise IndexError("tree %d of %d" % (t, self.n_trees))
        _, node, lo, hi = self._sides[t]
        return node.astype(np.int64), (hi - lo).astype(np.int64), None if self._frequency is None else self._frequency[t]

    def to_dataframe(self):
        """One row per pair of the range as a pandas DataFrame (pandas imported here)."""
        import pandas as pd
        frame = pd.DataFrame({k: getattr(self, k) for k in self.COLUMNS})
        frame.insert(2, "name_i", [self.names[v] for v in self.i])
        frame.insert(3, "name_j", [self.names[v] for v in self.j])
        return frame


def tree_set(trees, leaves=None, rooted=False, min_branch=None, begin=0, count=None, frequencies=True, device=..., chunk_tasks=0):
    """Every two trees of a set compared by the clades they share, in one pass: the Robinson-Foulds distance between every
    two of them and, per clade, the number of trees that hold it (Felsenstein's count for every tree of the set at once:
    what a majority-rule consensus is read from).

    ``trees``: a sequence of :class:`SuchTree` objects, Newick texts, paths to Newick files, :class:`Dendrogram`s or flat
    trees; texts and paths are parsed into flat arrays only.  ``leaves``: None = the names every tree holds, else a list
    of names -- a tree that lacks one is a ValueError naming the tree and the leaf; 4 to 16384 of them.  ``rooted`` and
    ``min_branch`` as in :meth:`SuchTree.compare_clades`: one :func:`clade_side` per tree.  ``begin`` / ``count``: a range
    of the triangle of pairs k = i (i - 1) / 2 + j, j < i (``count=None``: to its end).  ``frequencies``: also count, per
    clade, the trees that hold it (whole triangle only).  ``device``: None runs the host restatement, an index the kernel
    on that device -- the same integers; ... takes the host while pairs x leaves is below RF_DEVICE_MIN_WORK and device 0 from there.
    Returns a :class:`TreeSetComparison`.  An extension: the reference has no counterpart.
    """
    from . import _capi
    from .suchtree import int_arg
    flats = []
    for t, tree in enumerate(trees):
        flat = read_flat_tree(tree, extended=True)
        if flat is None:
            raise TypeError("tree %d must be a SuchTree, a Newick text, a path, a Dendrogram or a flat tree" % t)
        flats.append(flat)
    if not flats:
        raise ValueError("no trees")
    if leaves is None:
        common = set(flats[0].leaves)
        for flat in flats[1:]:
            common &= set(flat.leaves)
        names = [name for name, _ in sorted(flats[0].leaves.items(), key=lambda kv: kv[1]) if name in common]
    else:
        names = list(leaves)
    m = len(names)
    if m < 4 or m > _capi.RF_MAX_LEAVES:
        raise ValueError("%d common leaves: 4 to %d" % (m, _capi.RF_MAX_LEAVES))
    rooted = bool(rooted)
    sides = []
    for t, flat in enumerate(flats):
        where = flat.leaves
        for name in names:
            if name not in where:
                raise ValueError("tree %d has no leaf %r" % (t, name))
        ids = np.fromiter((where[name] for name in names), dtype=np.int64, count=m)
        sides.append(clade_side(flat, ids, rooted, min_branch))
    total = len(flats) * (len(flats) - 1) // 2
    begin = int_arg("begin", begin)
    count = total - begin if count is None else int_arg("count", count)
    if begin > total or count < 0 or count > total - begin:
        raise ValueError("pairs [%d, +%d) of a triangle of %d" % (begin, count, total))
    whole = begin == 0 and count == total
    shared, counts = _capi.rf_tasks(m, *_rf_sides(sides, m), rooted=rooted, begin=begin, count=count, want_count=bool(frequencies) and whole,
                                    device=_rf_device(device, count, m), chunk_tasks=int_arg("chunk_tasks", chunk_tasks))
    return TreeSetComparison(sides, m, rooted, begin, shared, counts, names)


class RelabelledRF:
    """The Robinson-Foulds half of the topology test in one call (:func:`rf_relabelled`): ``rf``, ``shared``, ``n_a``,
    ``n_b`` of the two trees as aligned, ``perm_rf`` (int64, in draw order; None without ``keep_stats``), ``n_le`` = the
    relabellings with rf_p <= rf and ``p_value`` = (n_le + 1) / (permutations + 1); ``rooted``, ``permutations``, ``seed``,
    ``stream`` and ``n`` repeat the run.  Unpacks as ``rf, p, n = result``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.rf, self.p_value, self.n))

    def __repr__(self):
        return "RelabelledRF(rf=%d, p_value=%r, n=%d, permutations=%d)" % (self.rf, self.p_value, self.n, self.permutations)


def rf_relabelled(flat_a, ids_a, flat_b, ids_b, permutations=999, seed=None, stream=0, rooted=True, min_branch=None, keep_stats=True, device=...,
                  chunk_tasks=0):
    """The Robinson-Foulds distance of two flat trees over aligned leaf-id lists (leaf k is ``ids_a[k]`` in A and
    ``ids_b[k]`` in B) against B relabelled, every relabelling in one batch.

    Relabelling p = 1 .. permutations is sigma_p = ``hommola_permutation(seed, stream, p, 0, n)``, numbered as
    :func:`dendrogram_congruence` numbers them: leaf sigma_p[k] of B is aligned with leaf k of A.  With A the tree and B
    the dendrogram this is that test's ``rf``, ``perm_rf`` and ``n_le``.  Both :func:`clade_side`s are built once; the
    alignment rows are generated on the host (4 n bytes each).  ``device`` as in :func:`tree_set`, the tasks being the
    relabellings and the observed pair.  Returns a :class:`RelabelledRF`.
    """
    from . import _capi
    from .suchtree import int_arg, seed_arg
    permutations, stream = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1"), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1")
    seed = seed_arg(seed)
    ids_a, ids_b = (np.ascontiguousarray(v, dtype=np.int64) for v in (ids_a, ids_b))
    if ids_a.ndim != 1 or ids_a.shape != ids_b.shape:
        raise ValueError("the two id lists must be 1-D and of equal length")
    n = len(ids_a)
    if n < 4 or n > _capi.RF_MAX_LEAVES:
        raise ValueError("%d leaves: 4 to %d" % (n, _capi.RF_MAX_LEAVES))
    rooted = bool(rooted)
    sides = [clade_side(flat_a, ids_a, rooted, min_branch), clade_side(flat_b, ids_b, rooted, min_branch)]
    align = np.empty((permutations, n), dtype=np.int32)
    for p in range(1, permutations + 1):
        align[p - 1] = hommola_permutation(seed, stream, p, 0, n)
    tasks = permutations + 1
    task_p = np.arange(-1, permutations, dtype=np.int32)
    shared, _ = _capi.rf_tasks(n, *_rf_sides(sides, n), rooted=rooted, align=align if permutations else None, task_i=np.zeros(tasks, dtype=np.int32),
                               task_j=np.ones(tasks, dtype=np.int32), task_p=task_p, want_count=False, device=_rf_device(device, tasks, n),
                               chunk_tasks=int_arg("chunk_tasks", chunk_tasks))
    n_a, n_b = len(sides[0][1]), len(sides[1][1])
    rf_all = n_a + n_b - 2 * shared.astype(np.int64)
    rf, perm_rf = int(rf_all[0]), rf_all[1:]
    n_le = int((perm_rf <= rf).sum())
    return RelabelledRF(rf=rf, shared=int(shared[0]), n_a=n_a, n_b=n_b, perm_rf=perm_rf if keep_stats else None, n_le=n_le,
                        p_value=(n_le + 1) / (permutations + 1), rooted=rooted, permutations=permutations, seed=seed, stream=stream, n=n)


def null_summary(observed, null, degenerate=None):
    """(mean, sd, ses, n_le) per row of ``null`` (rows, draws) against ``observed`` (rows): NaN draws left out, sd with
    ddof = 1, exactly 0 where all draws are equal; rows marked ``degenerate`` have the observation as their null."""
    import warnings
    rows, draws = null.shape
    mean, sd = np.full(rows, np.nan), np.full(rows, np.nan)
    n_le = np.zeros(rows, dtype=np.int64)
    if draws:
        with np.errstate(invalid="ignore", divide="ignore"):
            with warnings.catch_warnings():      # (a row of NaN draws only: numpy warns and gives NaN, which is the answer)
                warnings.simplefilter("ignore", RuntimeWarning)
                mean = np.nanmean(null, axis=1)
                sd = np.nanstd(null, axis=1, ddof=1)
                top = np.nanmax(null, axis=1)
                flat = top == np.nanmin(null, axis=1)
            mean = np.where(flat, top, mean)
            sd = np.where(flat & (np.count_nonzero(~np.isnan(null), axis=1) >= 2), 0.0, sd)
            n_le = np.count_nonzero(null <= observed[:, None], axis=1)
    if degenerate is not None and draws:
        mean = np.where(degenerate, observed, mean)
        sd = np.where(degenerate, 0.0, sd)
        n_le = np.where(degenerate & ~np.isnan(observed), draws, n_le)
    with np.errstate(invalid="ignore", divide="ignore"):
        ses = np.where(sd > 0, (observed - mean) / sd, np.nan)
    return mean, sd, ses, n_le


QUARTET_MAX_ALL = 1 << 36      # SuchTree.compare_quartets(samples=None) enumerates at most this many quartets


@dataclass(frozen=True)
class QuartetComparison:
    """How two trees resolve the same n quartets (SuchTree.compare_quartets).

    ``table[i, j]`` (int64, 4 x 4) counts the quartets of class i in the first tree and class j in the second: class 0
    is ab|cd, 1 ac|bd, 2 ad|bc of the quartet (a, b, c, d) and 3 "unresolved" -- no MRCA of its six pairs is unique,
    which four distinct leaves never give (repeated ids and internal nodes may).  ``agree`` is the trace over classes
    0..2, ``unresolved`` the sum of row and column 3, ``similarity`` = agree / n and ``distance`` = 1 - similarity: over
    all quartets of a leaf set (``mode`` "all") the normalised quartet distance.  ``stderr`` = sqrt(s (1 - s) / n), the
    binomial standard error of ``similarity`` for a sample (``mode`` "sample"), 0.0 for all quartets; for explicit
    quartets (``mode`` "given") it is that of a sample, should the rows be one.  ``n_leaves`` is the length of the leaf
    list (None for explicit quartets), ``seed`` the seed of a sample (None otherwise): quartet k of it is
    ``quartet_positions(n_leaves, samples, seed)[k]``.  The counts are exact integers.
    """

    n: int
    table: np.ndarray
    n_leaves: Optional[int] = None
    mode: str = "given"
    seed: Optional[int] = None

    def __post_init__(self):
        t = np.asarray(self.table, dtype=np.int64)
        if t.shape != (4, 4):
            raise ValueError("table must be 4 x 4")
        if int(t.sum()) != int(self.n):
            raise ValueError("n must be the sum of the table")
        if self.mode not in ("all", "sample", "given"):
            raise ValueError("mode must be 'all', 'sample' or 'given'")
        object.__setattr__(self, "table", t)
        object.__setattr__(self, "n", int(self.n))

    @classmethod
    def from_table(cls, table, n_leaves=None, mode="given", seed=None):
        table = np.asarray(table, dtype=np.int64)
        return cls(n=int(table.sum()), table=table, n_leaves=n_leaves, mode=mode, seed=seed)

    @property
    def agree(self) -> int:
        return int(self.table[0, 0] + self.table[1, 1] + self.table[2, 2])

    @property
    def unresolved(self) -> int:
        return int(self.table[3, :].sum() + self.table[:3, 3].sum())

    @property
    def similarity(self) -> float:
        return self.agree / self.n if self.n else float("nan")

    @property
    def distance(self) -> float:
        return 1.0 - self.similarity

    @property
    def stderr(self) -> float:
        if self.n == 0:
            return float("nan")
        if self.mode == "all":
            return 0.0
        s = self.similarity
        return math.sqrt(s * (1.0 - s) / self.n)

    @classmethod
    def merge(cls, a: "QuartetComparison", b: "QuartetComparison") -> "QuartetComparison":
        """Add the tables of two results over disjoint quartet ranges of the same question: the counts are integers, so
        the sum is the table of the union whatever the split.  ``n_leaves``, ``mode`` and ``seed`` are kept where both
        parts agree (else None, and mode "given")."""
        return cls(n=a.n + b.n, table=a.table + b.table, n_leaves=a.n_leaves if a.n_leaves == b.n_leaves else None,
                   mode=a.mode if a.mode == b.mode else "given", seed=a.seed if a.seed == b.seed else None)


def quartet_positions(m, samples=None, seed=0, begin=0, count=None, device=None):
    """The int32 (count, 4) leaf positions of the quartets SuchTree.compare_quartets compares over a list of ``m``
    leaves: with ``samples=None`` quartets [begin, begin + count) of all C(m,4) in colexicographic order (count None: up
    to the last), else quartets [begin, begin + count) of the sample drawn from ``seed`` (count None: up to ``samples``;
    quartet k depends on (seed, k, m) alone).  ``device=None`` computes them on the host, without a GPU; a device index
    runs the generator kernel there -- the same values."""
    from . import _capi
    m, begin = int(m), int(begin)
    if samples is None:
        mode = "all"
        if count is None:
            if m > _capi.QUARTET_MAX_LEAVES_ALL:
                raise ValueError("all quartets of %d leaves: at most %d leaves; give samples=" % (m, _capi.QUARTET_MAX_LEAVES_ALL))
            count = (math.comb(m, 4) if m >= 4 else 0) - begin
    else:
        mode = "sample"
        if count is None:
            count = int(samples) - begin
    return _capi.quartet_positions(mode, 0 if samples is None else seed, m, begin, count, -1 if device is None else int(device))


MANTEL_METHODS = ("pearson", "spearman")
MANTEL_ALTERNATIVES = ("two-sided", "greater", "less")


class MantelResult:
    """The Mantel test, or the partial Mantel test given a third matrix (mantel, SuchTree.mantel,
    SuchLinkedTrees.phylosymbiosis).

    ``corr_coeff`` is the correlation of the two matrices' ``n_pairs`` = n (n - 1) / 2 off-diagonal entries -- Pearson's r
    of the values or, with ``method="spearman"``, of their midranks; with a third matrix the partial correlation of x
    and y given z -- and ``p_value`` = (count + 1) / (permutations + 1), the count being ``n_ge`` (permuted statistic >=
    the observed one), ``n_le`` or ``n_abs_ge`` by ``alternative`` ("greater", "less", "two-sided").  The matrices enter
    the sums as int32 codes (``shift_x`` / ``shift_y`` / ``shift_z``: the fixed point of the Pearson form, None for
    ranks), so ``sxy`` -- and ``sxz`` -- of every permutation and the invariant ``sx``, ``sy``, ``sz``, ``sxx``, ``syy``,
    ``szz``, ``syz`` are exact Python ints: in the simple test the three counts compare integers.  ``perm_stats`` is the
    float64 statistic of each permutation in draw order with ``keep_stats=True``, else None.  A constant matrix gives NaN
    for both.  ``seed`` repeats the run.  Unpacks as ``r, p, n = result``, as scikit-bio's ``mantel`` returns.
    ``leaves`` / ``names`` / ``measure`` are filled in by ``phylosymbiosis``.
    """

    def __init__(self, **kw):
        self.leaves = self.names = self.measure = None
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.corr_coeff, self.p_value, self.n))

    def __repr__(self):
        return "MantelResult(corr_coeff=%r, p_value=%r, n=%d, method=%r, alternative=%r, permutations=%d)" % (
            self.corr_coeff, self.p_value, self.n, self.method, self.alternative, self.permutations)


def mantel_condensed(a, name="x", least=3):
    """(the float64 condensed form of ``a`` in the triangle order k = i (i - 1) / 2 + j, j < i; n): ``a`` is a square
    symmetric (n, n) matrix, whose diagonal is ignored, or already condensed.  ValueError, naming the offender, for a
    NaN or an infinity, a cell whose mirror differs, a length that is no triangle, n < ``least`` or n > 16384."""
    from . import _capi
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        if a.shape[0] != a.shape[1]:
            raise ValueError("%s: a %d x %d matrix is not square" % ((name,) + a.shape))
        n = int(a.shape[0])
    elif a.ndim == 1:
        n = (1 + math.isqrt(1 + 8 * len(a))) // 2
        if n * (n - 1) // 2 != len(a):
            raise ValueError("%s: %d values are not the n (n - 1) / 2 pairs of any n" % (name, len(a)))
    else:
        raise ValueError("%s must be a square matrix or a condensed vector" % name)
    if n < least or n > _capi.HOMMOLA_MAX_UNIVERSE:
        raise ValueError("%s: n = %d objects: %d to %d" % (name, n, least, _capi.HOMMOLA_MAX_UNIVERSE))
    if a.ndim == 1:
        bad = np.flatnonzero(~np.isfinite(a))
        if len(bad):
            raise ValueError("%s[%d] = %r is not finite" % (name, int(bad[0]), float(a[bad[0]])))
        return np.ascontiguousarray(a), n
    i, j = np.tril_indices(n, -1)      # (row-major over the lower triangle: the triangle order)
    low, up = a[i, j], a[j, i]
    bad = np.flatnonzero(~(np.isfinite(low) & np.isfinite(up)))
    if len(bad):
        r, c = (int(i[bad[0]]), int(j[bad[0]])) if not np.isfinite(low[bad[0]]) else (int(j[bad[0]]), int(i[bad[0]]))
        raise ValueError("%s[%d][%d] = %r is not finite" % (name, r, c, float(a[r, c])))
    bad = np.flatnonzero(low != up)
    if len(bad):
        r, c = int(i[bad[0]]), int(j[bad[0]])
        raise ValueError("%s is not symmetric: %s[%d][%d] = %r, %s[%d][%d] = %r" % (name, name, r, c, float(a[r, c]), name, c, r, float(a[c, r])))
    return np.ascontiguousarray(low), n


def mantel_rank_codes(v):
    """The int32 Spearman codes of the m values ``v``: twice the midrank (1 .. m, ties averaged as
    scipy.stats.rankdata(v, "average") does, -0.0 tied with +0.0) minus (m + 1)."""
    v = np.asarray(v, dtype=np.float64) + 0.0      # (-0.0 + 0.0 is +0.0)
    _, inverse, counts = np.unique(v, return_inverse=True, return_counts=True)
    below = np.cumsum(counts) - counts
    return (2 * below + counts - len(v))[inverse.ravel()].astype(np.int32)      # (2 (below + (count + 1) / 2) - (m + 1))


def mantel_square(codes, n):
    """The (n, n) int32 matrix of condensed ``codes``, both triangles, a zero diagonal."""
    out = np.zeros((n, n), dtype=np.int32)
    i, j = np.tril_indices(n, -1)
    out[i, j] = out[j, i] = codes
    return out


def _mantel_ratio(num, den2):
    """num / sqrt(den2) of Python ints as float64; NaN where den2 <= 0"""
    return float("nan") if den2 <= 0 else num / math.sqrt(den2)


def mantel(x, y, z=None, method="pearson", permutations=999, seed=None, alternative="two-sided", stream=0, keep_stats=False, device=...,
           chunk_tasks=0):
    """The Mantel test of two distance matrices over the same n objects and, with ``z``, the partial Mantel test of x
    and y given z, the permutations on the GPU.

    Each of ``x``, ``y``, ``z`` is a square symmetric matrix (the diagonal is ignored) or a condensed vector in the
    project's triangle order k = i (i - 1) / 2 + j, j < i, as ``SetUniFrac.pair(k)`` gives it; 3 <= n <= 16384.
    ``method`` is "pearson" (the values, as fixed-point int32 codes with a shift per matrix: 30 bits of the largest
    value) or "spearman" (the midranks of the off-diagonal values, ranked here on the host).  Permutation p >= 1
    relabels the objects of x by ``hommola_permutation(seed, stream, p, 0, n)``, as vegan's ``mantel`` and
    ``mantel.partial`` do; every permuted sum is an exact integer computed on ``device`` (... = device 0; None = on the
    host, without a GPU: the same integers), so the first k permutations are the same for any ``permutations`` >= k and
    the counts behind the p-value have no floating-point ties.  ``seed=None`` draws a seed and reports it.
    ``chunk_tasks`` bounds a launch (0 = 2^20 tasks); no result depends on it.  Returns a :class:`MantelResult`.
    An extension: the reference has no counterpart.
    """
    from . import _capi
    from .suchtree import int_arg, seed_arg
    if method not in MANTEL_METHODS:
        raise ValueError("method must be one of %s" % (MANTEL_METHODS,))
    if alternative not in MANTEL_ALTERNATIVES:
        raise ValueError("alternative must be one of %s" % (MANTEL_ALTERNATIVES,))
    permutations, stream = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1"), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1")
    chunk_tasks, seed = int_arg("chunk_tasks", chunk_tasks), seed_arg(seed)
    vx, n = mantel_condensed(x, "x")
    given = [("x", vx)]
    for name, a in (("y", y), ("z", z)):
        if a is not None:
            v, n_a = mantel_condensed(a, name)
            if n_a != n:
                raise ValueError("%s has %d objects, x has %d" % (name, n_a, n))
            given.append((name, v))
    codes, shifts = {}, {"x": None, "y": None, "z": None}
    for name, v in given:
        if method == "spearman":
            codes[name] = mantel_rank_codes(v)
        else:
            codes[name], shifts[name] = _capi.mantel_quantise(v)
    dev = -1 if device is None else 0 if device is ... else int_arg("device", device)
    mom, rec = _capi.mantel_codes(mantel_square(codes["x"], n), codes["y"], codes.get("z"), permutations, seed, stream, dev, chunk_tasks)
    m = n * (n - 1) // 2
    sxy = _capi.mantel_ints(rec, "sxy")
    var_x, var_y = m * mom["sxx"] - mom["sx"] ** 2, m * mom["syy"] - mom["sy"] ** 2
    cxy = [m * s - mom["sx"] * mom["sy"] for s in sxy]      # m^2 cov(x_p, y): Python ints
    sums = dict(mom, sxy=sxy[0], sxz=None)
    if z is None:
        for k in ("sz", "szz", "syz"):
            sums[k] = None
        den = var_x * var_y
        r0 = _mantel_ratio(cxy[0], den)
        n_ge = sum(c >= cxy[0] for c in cxy[1:])
        n_le = sum(c <= cxy[0] for c in cxy[1:])
        n_abs_ge = sum(abs(c) >= abs(cxy[0]) for c in cxy[1:])
        stats = np.array([_mantel_ratio(c, den) for c in cxy[1:]], dtype=np.float64) if keep_stats else None
    else:
        sxz = _capi.mantel_ints(rec, "sxz")
        sums["sxz"] = sxz[0]
        var_z = m * mom["szz"] - mom["sz"] ** 2
        r_yz = _mantel_ratio(m * mom["syz"] - mom["sy"] * mom["sz"], var_y * var_z)
        r_xy = np.array([_mantel_ratio(c, var_x * var_y) for c in cxy], dtype=np.float64)
        r_xz = np.array([_mantel_ratio(m * s - mom["sx"] * mom["sz"], var_x * var_z) for s in sxz], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            den = (1.0 - r_xz * r_xz) * (1.0 - r_yz * r_yz)
            part = np.where(den > 0.0, (r_xy - r_xz * r_yz) / np.sqrt(np.where(den > 0.0, den, 1.0)), np.nan)
        r0 = float(part[0])
        n_ge = int(np.count_nonzero(part[1:] >= r0))
        n_le = int(np.count_nonzero(part[1:] <= r0))
        n_abs_ge = int(np.count_nonzero(np.abs(part[1:]) >= abs(r0)))
        stats = part[1:].copy() if keep_stats else None
    count = {"greater": n_ge, "less": n_le, "two-sided": n_abs_ge}[alternative]
    p_value = float("nan") if math.isnan(r0) else (count + 1) / (permutations + 1)
    return MantelResult(corr_coeff=r0, p_value=p_value, n=n, n_pairs=m, method=method, alternative=alternative, permutations=permutations,
                        seed=seed, stream=stream, n_ge=int(n_ge), n_le=int(n_le), n_abs_ge=int(n_abs_ge), perm_stats=stats, partial=z is not None,
                        shift_x=shifts["x"], shift_y=shifts["y"], shift_z=shifts["z"], **sums)


MANTEL_CORRECTIONS = ("holm", "bonferroni", None)


class MantelCorrelogram:
    """The Mantel correlogram of y over the distance classes of x (mantel_correlogram, SuchTree.mantel_correlogram,
    SuchLinkedTrees.phylosymbiosis_correlogram): at which distances of x are the objects' y values alike.

    One entry per class c, as numpy columns: ``breaks`` (K + 1 edges; class c holds breaks[c] <= x < breaks[c + 1], the
    last class its upper edge too), ``class_mid``, ``n_pairs`` (m_c), ``sums_q`` (the observed sum S_c of the int32 codes
    of y over the pairs of the class, int64; ``shift_y``: the fixed point of the Pearson form, None for ranks),
    ``corr_coeff`` (r_c = minus Pearson's r of the class indicator against y -- the values or, with
    ``method="spearman"``, their midranks: positive where the pairs of the class are more alike than average; NaN for an
    empty class, one that holds every pair, or a constant y), ``n_ge`` / ``n_le`` (the permutations whose r_c is >= /
    <= the observed one, counted on exact integers, ties in both), ``p_value`` (one-sided in the direction of the
    observed sign: (n_ge + 1) / (permutations + 1) where r_c >= 0, else with n_le), ``p_corrected`` (``correction``,
    ``progressive``) and ``tested`` (False: beyond the ``cutoff`` or a NaN class, both p NaN).  ``perm_stats`` is the
    float64 (permutations, K) matrix of r_c of each permutation in draw order with ``keep_stats=True``, else None.
    ``n`` objects; ``seed`` and ``stream`` repeat the run.  ``leaves`` / ``names`` / ``measure`` are filled in by the
    facades.
    """

    COLUMNS = ("class_mid", "n_pairs", "sums_q", "corr_coeff", "n_ge", "n_le", "p_value", "p_corrected", "tested")

    def __init__(self, **kw):
        self.leaves = self.names = self.measure = None
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.class_mid)

    def row(self, c):
        """class ``c`` as a dict: its edges and its entry of every column"""
        c = range(len(self))[c]
        out = {"lower": float(self.breaks[c]), "upper": float(self.breaks[c + 1])}
        out.update((k, getattr(self, k)[c].item()) for k in self.COLUMNS)
        return out

    def to_dataframe(self):
        """one row per class: lower, upper and the columns"""
        import pandas as pd
        return pd.DataFrame(dict({"lower": self.breaks[:-1], "upper": self.breaks[1:]}, **{k: getattr(self, k) for k in self.COLUMNS}))

    def __repr__(self):
        return "MantelCorrelogram(n=%d, classes=%d, tested=%d, method=%r, permutations=%d)" % (
            self.n, len(self), int(np.count_nonzero(self.tested)), self.method, self.permutations)


def mantel_classes(x, breaks):
    """The uint8 class of each value of ``x`` under the K + 1 increasing edges ``breaks``: class c holds breaks[c] <= x
    < breaks[c + 1], the last class its upper edge too; a value outside all classes gets ST_CLASS_NONE (255)."""
    from . import _capi
    x, breaks = np.asarray(x, dtype=np.float64), np.asarray(breaks, dtype=np.float64)
    K = len(breaks) - 1
    c = np.searchsorted(breaks, x, side="right") - 1
    c[x == breaks[-1]] = K - 1
    c[(x < breaks[0]) | (x > breaks[-1])] = _capi.CLASS_NONE
    return c.astype(np.uint8)


def mantel_adjust(p, correction="holm", progressive=True):
    """The p-values ``p`` of the tested classes, in class order, corrected for multiple tests: "bonferroni" (t p, at
    most 1), "holm" (step-down: with p sorted, adj_(i) = max over j <= i of min(1, (t - j + 1) p_(j))) or None.
    ``progressive``: the k-th value is corrected within the first k (t = k), as Legendre & Legendre describe for a
    correlogram; else every value within all of them."""
    if correction not in MANTEL_CORRECTIONS:
        raise ValueError("correction must be one of %s" % (MANTEL_CORRECTIONS,))
    p = np.asarray(p, dtype=np.float64)

    def within(q):      # every value of q corrected within q
        t = len(q)
        if correction is None or t == 0:
            return q.copy()
        if correction == "bonferroni":
            return np.minimum(1.0, t * q)
        order = np.argsort(q, kind="stable")
        adj = np.maximum.accumulate(np.minimum(1.0, (t - np.arange(t)) * q[order]))
        out = np.empty(t, dtype=np.float64)
        out[order] = adj
        return out
    if not progressive:
        return within(p)
    return np.array([within(p[:k + 1])[k] for k in range(len(p))], dtype=np.float64)


def _sum_of_squares(codes):
    """sum of codes^2 of int32 codes as a Python int: three int64 sums that cannot overflow below 2^27 codes"""
    v = codes.astype(np.int64)
    hi, lo = v >> 16, v & 0xFFFF      # v = hi 2^16 + lo, |hi| <= 2^15, 0 <= lo < 2^16
    return (int((hi * hi).sum()) << 32) + (int((hi * lo).sum()) << 17) + int((lo * lo).sum())


def mantel_correlogram(x, y, n_classes=None, breaks=None, cutoff=True, method="pearson", permutations=999, seed=None, stream=0,
                       correction="holm", progressive=True, keep_stats=False, device=..., chunk_tasks=0):
    """The Mantel correlogram (Oden & Sokal 1986; Legendre & Legendre 2012; vegan's ``mantel.correlog``): the pairs of n
    objects are cut into classes of ``x``, and every class gets a Mantel statistic of ``y`` against the class indicator
    with a permutation test of its own -- all classes in one pass over the pairs on the GPU.

    ``x`` and ``y`` are read as :func:`mantel` reads them (square symmetric or condensed, 3 <= n <= 16384); y enters as
    int32 codes by ``method`` ("pearson": fixed point; "spearman": midranks).  Classes: ``breaks`` are the K + 1
    increasing edges -- class c holds breaks[c] <= x < breaks[c + 1], the last class its upper edge too, a pair outside
    all classes is in none -- by default ``n_classes`` equal-width classes from min(x) to max(x), and ``n_classes=None``
    is Sturges' rule K = ceil(1 + log2(m)) over the m = n (n - 1) / 2 pairs; at most 64 classes.  Permutation p >= 1
    relabels the objects of x -- hence the classes -- by ``hommola_permutation(seed, stream, p, 0, n)``, the permutations
    of :func:`mantel`.  With m_c pairs in class c and S_c(p) the exact integer sum of the codes of y over the relabelled
    class, r_c = -Pearson(indicator_c, y) = -(m S_c - m_c Sy) / sqrt(m_c (m - m_c) (m Syy - Sy^2)), positive where the
    pairs of the class are more alike than average.  r_c falls strictly as S_c rises, so the counts compare integers:
    ``n_ge[c]`` is the number of p >= 1 with S_c(p) <= S_c(0), ``n_le[c]`` that with S_c(p) >= S_c(0); a relabelling
    that maps the classes onto themselves ties and is counted in both.  ``p_value[c]`` is one-sided in the direction of
    the observed sign: (n_ge + 1) / (permutations + 1) where r_c >= 0, else (n_le + 1) / (permutations + 1).

    ``cutoff=True`` tests class c only when its upper edge is at most the smallest, over the objects, of an object's
    largest x -- the distances every object takes part in; the classes beyond keep ``corr_coeff`` and their sums, with
    ``tested`` False and p NaN.  ``cutoff=False`` tests every class with 0 < m_c < m.  ``correction`` ("holm",
    "bonferroni", None) and ``progressive`` are those of :func:`mantel_adjust`, over the tested classes in class order.
    ``device``, ``seed``, ``stream``, ``keep_stats`` and ``chunk_tasks`` are those of :func:`mantel`.

    These are this library's definitions: close to vegan's ``mantel.correlog``, and not claimed to reproduce its
    p-values.  Returns a :class:`MantelCorrelogram`.  An extension: the reference has no counterpart.
    """
    from . import _capi
    from .suchtree import int_arg, seed_arg
    if method not in MANTEL_METHODS:
        raise ValueError("method must be one of %s" % (MANTEL_METHODS,))
    if correction not in MANTEL_CORRECTIONS:
        raise ValueError("correction must be one of %s" % (MANTEL_CORRECTIONS,))
    permutations, stream = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1"), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1")
    chunk_tasks, seed = int_arg("chunk_tasks", chunk_tasks), seed_arg(seed)
    vx, n = mantel_condensed(x, "x")
    vy, n_y = mantel_condensed(y, "y")
    if n_y != n:
        raise ValueError("y has %d objects, x has %d" % (n_y, n))
    m = n * (n - 1) // 2
    if breaks is None:
        K = math.ceil(1 + math.log2(m)) if n_classes is None else int_arg("n_classes", n_classes)
        if K < 1:
            raise ValueError("n_classes must be at least 1")
        lo, hi = float(vx.min()), float(vx.max())
        if K <= _capi.CLASS_MAX and not lo < hi:
            raise ValueError("x is constant: no distance classes")
        edges = np.linspace(lo, hi, K + 1) if K <= _capi.CLASS_MAX else None
    else:
        edges = np.array(breaks, dtype=np.float64)
        if edges.ndim != 1 or len(edges) < 2 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
            raise ValueError("breaks must be at least two finite, strictly increasing edges")
        K = len(edges) - 1
        if n_classes is not None and int(n_classes) != K:
            raise ValueError("n_classes = %d, breaks give %d classes" % (int(n_classes), K))
    if K > _capi.CLASS_MAX:
        raise ValueError("%d classes: at most %d" % (K, _capi.CLASS_MAX))
    cls = mantel_classes(vx, edges)
    if method == "spearman":
        codes, shift = mantel_rank_codes(vy), None
    else:
        codes, shift = _capi.mantel_quantise(vy)
    dev = -1 if device is None else 0 if device is ... else int_arg("device", device)
    sums = _capi.class_sums_codes(codes, cls, K, permutations, seed, stream, dev, chunk_tasks)
    m_c = np.bincount(cls, minlength=256)[:K].astype(np.int64)
    sy, syy = int(codes.sum(dtype=np.int64)), _sum_of_squares(codes)
    var_y = m * syy - sy * sy
    obs = [int(v) for v in sums[0].tolist()]
    sizes = [int(v) for v in m_c.tolist()]
    num = [m * s - mc * sy for s, mc in zip(obs, sizes)]      # m^2 cov(indicator_c, y): Python ints
    den = [mc * (m - mc) * var_y for mc in sizes]
    corr = np.array([_mantel_ratio(-a, d) for a, d in zip(num, den)], dtype=np.float64)
    n_ge = np.count_nonzero(sums[1:] <= sums[0], axis=0).astype(np.int64)
    n_le = np.count_nonzero(sums[1:] >= sums[0], axis=0).astype(np.int64)
    tested = ~np.isnan(corr)
    if cutoff:      # the largest x of every object, row by row of the triangle
        reach = np.full(n, -np.inf)
        for i in range(1, n):
            seg = vx[i * (i - 1) // 2:i * (i + 1) // 2]
            reach[i] = max(reach[i], seg.max())
            np.maximum(reach[:i], seg, out=reach[:i])
        tested &= edges[1:] <= reach.min()
    count = np.where(np.array([a <= 0 for a in num]), n_ge, n_le)
    p_value = np.where(tested, (count + 1) / (permutations + 1), np.nan)
    p_corrected = np.full(K, np.nan)
    p_corrected[tested] = mantel_adjust(p_value[tested], correction, progressive)
    stats = None
    if keep_stats:
        stats = np.full((permutations, K), np.nan)
        for c in range(K):
            if den[c] > 0:
                root = math.sqrt(den[c])
                stats[:, c] = [-(m * int(s) - sizes[c] * sy) / root for s in sums[1:, c].tolist()]
    return MantelCorrelogram(breaks=edges, class_mid=(edges[:-1] + edges[1:]) / 2, n_pairs=m_c, sums_q=sums[0].copy(), corr_coeff=corr, n_ge=n_ge,
                             n_le=n_le, p_value=p_value, p_corrected=p_corrected, tested=tested, n=n, method=method, permutations=permutations,
                             seed=seed, stream=stream, shift_y=shift, perm_stats=stats, correction=correction, progressive=bool(progressive),
                             cutoff=bool(cutoff))


GROUP_TESTS = ("permanova", "anosim")


class GroupTestResult:
    """PERMANOVA or ANOSIM of a distance matrix against a grouping of its objects (permanova, anosim,
    SuchLinkedTrees.partner_group_differences).

    ``statistic`` is the pseudo-F of ``method`` "permanova" (with ``r2`` = 1 - SS_W / SS_T) or Clarke's R of "anosim"
    (``r2`` None), ``p_value`` = (``n_ge`` + 1) / (``permutations`` + 1), ``n_ge`` the permutations whose statistic is
    >= the observed one -- counted on exact integers.  ``n`` objects fall in ``n_groups`` groups of ``group_sizes``,
    named by ``labels`` in the same order.  ``within_q`` holds the observed within-group sum of the int32 codes of each
    group as Python ints (``shift``: the fixed point of the squared distances; None for ranks).  ``perm_stats`` is the
    float64 statistic of each permutation in draw order with ``keep_stats=True``, else None.  ``seed`` repeats the run.
    Unpacks as ``stat, p, n = result``.  ``leaves`` / ``names`` / ``measure`` / ``dropped`` are filled in by
    ``partner_group_differences``.
    """

    def __init__(self, **kw):
        self.leaves = self.names = self.measure = self.dropped = None
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.statistic, self.p_value, self.n))

    def __repr__(self):
        return "GroupTestResult(method=%r, statistic=%r, p_value=%r, n=%d, n_groups=%d, permutations=%d)" % (
            self.method, self.statistic, self.p_value, self.n, self.n_groups, self.permutations)


def group_codes(grouping, n):
    """(labels in order of first appearance, the uint8 code of each of the ``n`` objects, group sizes).  ValueError for
    a grouping that is not one label per object, one group, every object alone, or more than 256 groups."""
    from . import _capi
    grouping = list(grouping)
    if len(grouping) != n:
        raise ValueError("grouping holds %d labels for %d objects" % (len(grouping), n))
    index = {}
    codes = np.array([index.setdefault(g, len(index)) for g in grouping], dtype=np.int64)
    a = len(index)
    if a == 1:
        raise ValueError("every object is in one group")
    if a == n:
        raise ValueError("every object is alone in its group")
    if a > _capi.GROUP_MAX:
        raise ValueError("%d groups: at most %d" % (a, _capi.GROUP_MAX))
    return list(index), codes.astype(np.uint8), np.bincount(codes, minlength=a).tolist()


def _ratio(num, den):
    """num / den of Python ints as float64: inf, -inf or NaN where den is 0"""
    if den == 0:
        return float("nan") if num == 0 else math.copysign(float("inf"), num)
    return num / den


def group_weighted_sums(sums, weights, python_ints=None):
    """[sum over the groups g of sums[p][g] * weights[g] for p] as Python ints: in int64 numpy where a groups of
    |sum| < 2^58 times the largest weight stay below 2^63, else -- or with ``python_ints=True`` -- in Python ints."""
    if python_ints is None:
        python_ints = len(weights) * (1 << 58) * max(weights) >= (1 << 63)
    if python_ints:
        T = sums.astype(object) @ np.array(weights, dtype=object)
    else:
        T = sums @ np.array(weights, dtype=np.int64)
    return [int(t) for t in T.tolist()]


def _group_test(method, d, grouping, permutations, seed, stream, keep_stats, device, chunk_tasks):
    from . import _capi
    from .suchtree import int_arg, seed_arg
    permutations, stream = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1"), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1")
    chunk_tasks, seed = int_arg("chunk_tasks", chunk_tasks), seed_arg(seed)
    v, n = mantel_condensed(d, "d")
    labels, g, sizes = group_codes(grouping, n)
    a, m = len(labels), n * (n - 1) // 2
    n_within = sum(s * (s - 1) // 2 for s in sizes)
    if method == "anosim" and (n_within == 0 or n_within == m):
        raise ValueError("no within-group pair or no between-group pair")
    if method == "permanova":
        y, shift = _capi.mantel_quantise(v * v)
    else:
        y, shift = mantel_rank_codes(v), None
    dev = -1 if device is None else 0 if device is ... else int_arg("device", device)
    sums = _capi.group_sums_codes(y, g, a, permutations, seed, stream, dev, chunk_tasks)
    r2 = None
    if method == "permanova":
        lcm = math.lcm(*sizes)
        T = group_weighted_sums(sums, [lcm // s for s in sizes])      # L SS_W in code units
        total = int(y.sum(dtype=np.int64))    # n SS_T
        # F = ((SS_T - SS_W) / (a - 1)) / (SS_W / (n - a)), SS_T = total / n, SS_W = T / L: one division of integers
        stat = lambda t: _ratio((total * lcm - t * n) * (n - a), (a - 1) * t * n)      # noqa: E731
        r2 = _ratio(total * lcm - T[0] * n, total * lcm)
        order = T
    else:
        S = [int(s) for s in sums.sum(axis=1).tolist()]
        between = n_within * (m - n_within)
        stat = lambda s: _ratio(-s, between)      # noqa: E731
        order = S
    statistic = stat(order[0])
    n_ge = sum(t <= order[0] for t in order[1:])      # (the statistic falls strictly as the within-group sum rises)
    stats = np.array([stat(t) for t in order[1:]], dtype=np.float64) if keep_stats else None
    p_value = float("nan") if math.isnan(statistic) else (n_ge + 1) / (permutations + 1)
    return GroupTestResult(statistic=statistic, p_value=p_value, n_ge=int(n_ge), n=n, n_groups=a, group_sizes=sizes, labels=labels,
                           within_q=[int(s) for s in sums[0].tolist()], shift=shift, method=method, permutations=permutations, seed=seed,
                           stream=stream, perm_stats=stats, r2=r2)


def permanova(d, grouping, permutations=999, seed=None, stream=0, keep_stats=False, device=..., chunk_tasks=0):
    """PERMANOVA (Anderson 2001; vegan's ``adonis2``, scikit-bio's ``permanova``): do the groups of ``grouping`` differ in
    the distances ``d`` between their n objects, the permutations on the GPU.

    ``d`` is a square symmetric matrix (the diagonal is ignored) or a condensed vector in the project's triangle order
    k = i (i - 1) / 2 + j, j < i; 3 <= n <= 16384.  ``grouping`` holds one hashable label per object: at least two
    groups, not every object alone, at most 256 groups.  The squared distances enter as fixed-point int32 codes (30 bits
    of the largest).  Permutation p >= 1 relabels the objects by ``hommola_permutation(seed, stream, p, 0, n)`` -- the
    permutations of ``mantel`` -- and the within-group sum of every group under every permutation is an exact integer
    computed on ``device`` (... = device 0; None = on the host, without a GPU: the same integers).  With the sum of a
    group divided by its size, L = the least common multiple of the sizes and T_p = sum over the groups of sum_g (L /
    n_g), the pseudo-F falls strictly as the integer T_p rises, so ``n_ge`` counts T_p <= T_0: the counts behind the
    p-value have no floating-point ties, and a relabelling that maps the groups onto themselves is counted, as it must
    be.  The first k permutations are the same for any ``permutations`` >= k.  ``seed=None`` draws a seed and reports
    it.  ``chunk_tasks`` bounds a launch (0 = 2^20 tasks); no result depends on it.  Returns a
    :class:`GroupTestResult`.  An extension: the reference has no counterpart.
    """
    return _group_test("permanova", d, grouping, permutations, seed, stream, keep_stats, device, chunk_tasks)


def anosim(d, grouping, permutations=999, seed=None, stream=0, keep_stats=False, device=..., chunk_tasks=0):
    """ANOSIM (Clarke 1993; vegan's and scikit-bio's ``anosim``): are the distances ``d`` between groups of
    ``grouping`` ranked above those within, the permutations on the GPU.

    The arguments and the permutations are those of :func:`permanova`.  The distances enter as their midranks (ties
    averaged, as scipy.stats.rankdata does), doubled and centred to int32 codes that sum to 0, so with S_p the sum of
    the codes over the within-group pairs under permutation p, N_W within-group pairs and N_B between, R_p = -S_p /
    (N_W N_B) is Clarke's (mean rank between - mean rank within) / (M / 2).  ``n_ge`` counts the integers S_p <= S_0: no
    floating-point ties.  Returns a :class:`GroupTestResult`.  An extension: the reference has no counterpart.
    """
    return _group_test("anosim", d, grouping, permutations, seed, stream, keep_stats, device, chunk_tasks)


PARAFIT_TRANSFORMS = ("sqrt", "none")


class ParaFitResult:
    """ParaFit (Legendre, Desdevises & Bazin 2002): the global test of cophylogeny and ParaFitLink1 of every link
    (parafit, SuchLinkedTrees.parafit).

    ``statistic`` is ParaFitGlobal, the trace of (C^T A B)(C^T A B)^T with B and C the principal coordinates of the two
    sides and A the link matrix, and ``p_value`` = (``n_ge`` + 1) / (``permutations`` + 1), ``n_ge`` counting the
    permutations whose trace is >= the observed one.  Both centred matrices enter as int32 codes (``shift_f``,
    ``shift_s``: the fixed point of the held and the shuffled side), so ``trace_q`` and ``link_stat_q`` are exact Python
    ints -- the float statistics are these times 2^-(shift_f + shift_s) -- and every count compares integers: a
    relabelling that maps the links onto themselves ties and is counted.

    Per link, in the order the links were given: ``link_stat`` is ParaFitLink1, the trace minus the trace without that
    link; ``link_n_ge`` counts the permutations p in which the statistic of the *relabelled* link l in the relabelled
    system, Link1_p(l), is >= the observed Link1_0(l), and ``link_p`` = (``link_n_ge`` + 1) / (``permutations`` + 1).
    This is this library's definition of the link test; it is not claimed to equal the link p-values of ape's
    ``parafit``.  ``link_f`` / ``link_s`` are the links' positions; ``link_a`` / ``link_b`` (TreeA / TreeB leaf ids)
    and ``link_names`` are filled in by ``SuchLinkedTrees.parafit``, as is ``shuffle``.  With ``test_links=False`` the
    two link-test fields are None.  With ``keep_stats=True``, ``perm_stats`` is the float64 trace of each permutation
    in draw order and ``perm_link_stats`` the (permutations, n_links) Link1_p values; else both are None.
    ``transform`` is "sqrt" (the distances themselves are centred) or "none" (the squared distances).  ``seed``
    repeats the run.  Unpacks as ``stat, p, n = result`` with n = ``n_links``.
    """

    def __init__(self, **kw):
        self.shuffle = self.link_a = self.link_b = self.link_names = None
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.statistic, self.p_value, self.n_links))

    def __len__(self):
        return self.n_links

    def __repr__(self):
        return "ParaFitResult(statistic=%r, p_value=%r, n_links=%d, transform=%r, permutations=%d)" % (
            self.statistic, self.p_value, self.n_links, self.transform, self.permutations)

    def row(self, l) -> dict:
        """The fields of link ``l`` as a dict."""
        l = range(self.n_links)[l]
        out = {"link_f": int(self.link_f[l]), "link_s": int(self.link_s[l]), "link_stat": float(self.link_stat[l]), "link_stat_q": self.link_stat_q[l]}
        for k in ("link_a", "link_b", "link_n_ge", "link_p"):
            v = getattr(self, k)
            if v is not None:
                out[k] = v[l].item()
        if self.link_names is not None:
            out["link_names"] = self.link_names[l]
        return out

    def to_dataframe(self):
        """One row per link (pandas)."""
        import pandas as pd
        cols = {k: getattr(self, k) for k in ("link_a", "link_b", "link_f", "link_s", "link_stat", "link_n_ge", "link_p") if getattr(self, k) is not None}
        if self.link_names is not None:
            cols["name_a"], cols["name_b"] = [a for a, _ in self.link_names], [b for _, b in self.link_names]
        return pd.DataFrame(cols)


def parafit_centre(d, n, transform="sqrt"):
    """The float64 (n, n) Gower-centred matrix G = -1/2 J D2 J of the condensed distances ``d`` (triangle order): D2 is
    the distance itself with ``transform="sqrt"`` (the square root of the distances is what gets embedded) and its
    square with "none".  The lower triangle is mirrored, so G is symmetric bit for bit."""
    d2 = np.zeros((n, n), dtype=np.float64)
    i, j = np.tril_indices(n, -1)
    v = np.asarray(d, dtype=np.float64)
    d2[i, j] = d2[j, i] = v if transform == "sqrt" else v * v
    rows = d2.mean(axis=1)
    g = -0.5 * (d2 - rows[:, None] - rows[None, :] + d2.mean())
    g[j, i] = g[i, j]
    return g


def parafit(d_f, d_s, links, permutations=999, seed=None, shuffle_streams=None, transform="sqrt", test_links=True, keep_stats=False, device=...,
            chunk_tasks=0):
    """ParaFit of two distance matrices joined by links: the global statistic with its permutation test and
    ParaFitLink1 of every link with its own, in one pass over the link pairs on the GPU.

    ``d_f`` (the held side F) and ``d_s`` (the shuffled side S) are square symmetric matrices or condensed vectors, read
    as :func:`mantel` reads them; ``links`` is an (L, 2) array of (F position, S position), 3 to 16384 distinct links.
    Each matrix is Gower-centred in float64 on the host (G = -1/2 J D2 J) and quantised to int32 codes with a shift of
    its own.  With principal coordinates C C^T = G_s and B B^T = G_f, ParaFitGlobal = ||C^T A B||_F^2 is the sum of
    T[l][k] = G_f[f_l][f_k] G_s[s_l][s_k] over all link pairs, and ParaFitLink1(l) = 2 (row sum of T at l) - T[l][l]: no
    eigendecomposition is made.  ``transform="sqrt"`` (default) takes D2 = the distances themselves -- the embedding
    of their square roots (de Vienne et al. 2011), Euclidean for a tree metric, so the statistic is the PCoA definition's
    exactly; ``"none"`` takes D2 = the squared distances, and axes with negative eigenvalues enter with their sign (as
    vegan's ``betadisper`` treats them; ape's ``parafit`` drops them instead, so the two differ there).

    Permutation p >= 1 is Legendre's null: for every F position i with links separately, its partners are redrawn among
    the S positions -- ``sigma = hommola_permutation(seed, shuffle_streams[i], p, 0, n_s)``, link (f, s) becomes
    (f, sigma[s]).  Links of one F position keep distinct images; ``shuffle_streams`` (default: the F positions
    themselves) gives every F position its stream.  The link test compares Link1_p(l), the statistic of the relabelled
    link l in the relabelled system, with the observed Link1_0(l): see :class:`ParaFitResult`; it is not claimed to equal
    ape's link p-values.  All sums are exact integers computed on ``device`` (... = device 0; None = on the host, without
    a GPU: the same integers), the first k permutations are the same for any ``permutations`` >= k, and nothing depends on
    ``chunk_tasks`` (tasks per launch, 0 = 2^20).  ``seed=None`` draws a seed and reports it.  ParaFitLink2 is not
    computed.  An extension: the reference has no counterpart.
    """
    from . import _capi
    from .suchtree import int_arg, seed_arg
    if transform not in PARAFIT_TRANSFORMS:
        raise ValueError("transform must be one of %s" % (PARAFIT_TRANSFORMS,))
    permutations = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1")
    chunk_tasks, seed = int_arg("chunk_tasks", chunk_tasks), seed_arg(seed)
    v_f, n_f = mantel_condensed(d_f, "d_f")
    v_s, n_s = mantel_condensed(d_s, "d_s")
    links = np.asarray(links)
    if links.ndim != 2 or links.shape[1] != 2 or links.dtype.kind not in "iu":
        raise ValueError("links must be an (L, 2) integer array of (F position, S position)")
    L = int(links.shape[0])
    if L < 3 or L > _capi.HOMMOLA_MAX_UNIVERSE:
        raise ValueError("%d links: 3 to %d" % (L, _capi.HOMMOLA_MAX_UNIVERSE))
    links = links.astype(np.int64)
    for col, n, side in ((0, n_f, "F"), (1, n_s, "S")):
        bad = np.flatnonzero((links[:, col] < 0) | (links[:, col] >= n))
        if len(bad):
            raise ValueError("link %d: the %s position %d is outside the universe of %d" % (int(bad[0]), side, int(links[bad[0], col]), n))
    order = np.lexsort((links[:, 1], links[:, 0]))
    srt = links[order]
    same = np.flatnonzero((srt[1:] == srt[:-1]).all(axis=1))
    if len(same):
        raise ValueError("links %d and %d are the same link" % tuple(sorted((int(order[same[0]]), int(order[same[0] + 1])))))
    if shuffle_streams is None:
        streams = np.arange(n_f, dtype=np.int64)
    else:
        streams = np.asarray(shuffle_streams)
        if streams.shape != (n_f,) or streams.dtype.kind not in "iu" or (streams.astype(np.int64) < 0).any() or (streams.astype(np.int64) > 0x7FFFFFFF).any():
            raise ValueError("shuffle_streams must hold one non-negative int32 per F position")
    q_f, shift_f = _capi.mantel_quantise(parafit_centre(v_f, n_f, transform))
    q_s, shift_s = _capi.mantel_quantise(parafit_centre(v_s, n_s, transform))
    dev = -1 if device is None else 0 if device is ... else int_arg("device", device)
    total, obs, n_ge_l, every = _capi.parafit_codes(q_f, q_s, srt[:, 0], srt[:, 1], streams, permutations, seed, dev, chunk_tasks, keep=keep_stats)
    back = np.empty(L, dtype=np.int64)      # the caller's link k is sorted link back[k]
    back[order] = np.arange(L)
    scale = -(shift_f + shift_s)
    trace = _capi.parafit_ints(total)
    link_q = [_capi.parafit_ints(obs)[k] for k in back.tolist()]
    n_ge = sum(t >= trace[0] for t in trace[1:])
    perm_stats = perm_link_stats = None
    if keep_stats:
        perm_stats = np.array([math.ldexp(float(t), scale) for t in trace[1:]], dtype=np.float64)
        rows = _capi.parafit_ints(every[1:]) if permutations else []
        perm_link_stats = np.array([[math.ldexp(float(r[k]), scale) for k in back.tolist()] for r in rows], dtype=np.float64).reshape(permutations, L)
    return ParaFitResult(statistic=math.ldexp(float(trace[0]), scale), p_value=(n_ge + 1) / (permutations + 1), n_ge=int(n_ge), trace_q=trace[0],
                         perm_trace_q=trace[1:], shift_f=shift_f, shift_s=shift_s, n_links=L, n_f=n_f, n_s=n_s, permutations=permutations, seed=seed,
                         transform=transform, link_f=links[:, 0].copy(), link_s=links[:, 1].copy(), link_stat_q=link_q,
                         link_stat=np.array([math.ldexp(float(v), scale) for v in link_q], dtype=np.float64),
                         link_n_ge=n_ge_l[back].copy() if test_links else None,
                         link_p=(n_ge_l[back] + 1) / (permutations + 1) if test_links else None, perm_stats=perm_stats, perm_link_stats=perm_link_stats)


LINKAGE_METHODS = ("average", "single", "complete")
# compare.linkage(device=...) runs the host restatement below this n and the kernels on device 0 from it on: the n from
# which the device call beat the host restatement beyond both spreads (profiles/linkage_r32.log; README, "Dendrograms")
LINKAGE_DEVICE_MIN = 4096


def _linkage_device(device, n):
    """The ``device`` of _capi.linkage_codes for the ``device`` of a caller: ... follows LINKAGE_DEVICE_MIN."""
    from .suchtree import int_arg
    if device is ...:
        return 0 if n >= LINKAGE_DEVICE_MIN else -1
    return -1 if device is None else int_arg("device", device)


class Dendrogram:
    """An exact dendrogram of n objects (linkage, SuchLinkedTrees.partner_dendrogram): n - 1 merges in the order they were
    made, as scipy.cluster.hierarchy.linkage numbers them -- ids below n are objects, n + t is the cluster of merge t.

    ``left`` < ``right`` (int64) are the two clusters of a merge and ``size`` (int64) the objects -- with weights, the
    weight -- of the result; its value is the fraction ``num`` / ``den`` (int64: integers of the codes, not reduced),
    ``heights`` = ldexp(num / den, -shift) in float64, ``shift`` being the fixed point of the codes.  Heights never
    decrease; equal fractions are real ties, broken towards the lower slots (include/suchtree_hip.h, st_linkage_codes).
    ``Z`` is the (n - 1, 4) float64 array scipy's ``dendrogram``, ``fcluster`` and ``cophenet`` take.  ``leaves`` /
    ``names`` / ``measure`` are filled in by ``partner_dendrogram``.
    """

    def __init__(self, n, method, shift, rows):
        self.n, self.method, self.shift = int(n), method, shift
        self.left, self.right, self.size = (np.asarray(rows[k], dtype=np.int64).copy() for k in ("left", "right", "size"))
        self.num, self.den = np.asarray(rows["num"], dtype=np.int64).copy(), np.asarray(rows["den"], dtype=np.int64).copy()
        self.heights = np.array([math.ldexp(a / b, -(shift or 0)) for a, b in zip(self.num.tolist(), self.den.tolist())], dtype=np.float64)
        self.leaves = self.names = self.measure = None

    def __len__(self):
        return self.n - 1

    def __repr__(self):
        return "Dendrogram(n=%d, method=%r, shift=%r)" % (self.n, self.method, self.shift)

    @property
    def Z(self):
        return np.column_stack([self.left, self.right, self.heights, self.size]).astype(np.float64)

    def members(self, t):
        """The objects under merge ``t``, 0 <= t < n - 1, increasing."""
        t = int(t)
        if not 0 <= t < self.n - 1:
            raise IndexError("merge %d of %d" % (t, self.n - 1))
        out, stack = [], [self.n + t]
        while stack:
            c = stack.pop()
            if c < self.n:
                out.append(c)
            else:
                stack += (int(self.left[c - self.n]), int(self.right[c - self.n]))
        return sorted(out)

    def cophenetic(self):
        """The cophenetic distances -- the height of the merge that first joins two objects -- condensed in this
        library's pair order k = i (i - 1) / 2 + j, j < i."""
        n = self.n
        sq = np.zeros((n, n), dtype=np.float64)
        lists = [np.array([i]) for i in range(n)]
        for t, (l, r) in enumerate(zip(self.left.tolist(), self.right.tolist())):
            a, b = lists[l], lists[r]
            sq[np.ix_(a, b)] = sq[np.ix_(b, a)] = self.heights[t]
            lists.append(np.concatenate([a, b]))
            lists[l] = lists[r] = None
        i, j = np.tril_indices(n, -1)
        return sq[i, j]

    def _names(self, names):
        names = [str(i) for i in range(self.n)] if names is None else [str(v) for v in names]
        if len(names) != self.n or len(set(names)) != self.n:
            raise ValueError("names must be %d distinct names" % self.n)
        return names

    def to_newick(self, names=None):
        """The ultrametric tree as Newick text: the node of a merge sits at half its height, leaves at 0, a branch is
        the difference -- so two leaves are as far apart as the height of their merge.  ``names``: one per object
        (default "0", "1", ...); a name with Newick punctuation is quoted."""
        import re
        names = self._names(names)
        label = [v if re.fullmatch(r"[^\s()\[\],:;']+", v) else "'" + v.replace("'", "''") + "'" for v in names]
        n, half = self.n, (self.heights / 2.0).tolist()
        at = lambda c: 0.0 if c < n else half[c - n]      # noqa: E731
        out, stack = [], [(2 * n - 2, None, "")]      # (cluster, its parent, what follows it); a text alone is written out
        while stack:
            item = stack.pop()
            if isinstance(item, str):
                out.append(item)
                continue
            c, up, after = item
            tail = (";" if up is None else ":%r" % (at(up) - at(c))) + after
            if c < n:
                out.append(label[c] + tail)
            else:
                out.append("(")
                stack.append(")" + tail)
                stack.append((int(self.right[c - n]), c, ""))
                stack.append((int(self.left[c - n]), c, ","))
        return "".join(out)

    def to_flat(self, names=None):
        """The tree of :meth:`to_newick` as a FlatTree, through the Newick ingest: no GPU.  The ingest reads a zero length
        as epsilon, as the reference does for a polytomy; a dendrogram's zero is a tie -- two merges at one height --
        and is put back, so that ``min_branch=0.0`` of :func:`clade_side` finds it."""
        from .newick import EPSILON, flat_tree_from_newick
        flat = flat_tree_from_newick(self.to_newick(names))
        length = np.array(flat.distance, dtype=np.float32)
        length[length == np.float32(EPSILON)] = 0.0
        flat.distance = length
        return flat

    def to_tree(self, names=None, device=0):
        """The tree of :meth:`to_newick` as a :class:`SuchTree` on ``device``."""
        from .suchtree import SuchTree
        return SuchTree(self.to_flat(names), device=device)


def linkage(d, method="average", weights=None, device=...):
    """The exact dendrogram of a distance matrix: UPGMA (``method="average"``), single or complete linkage.

    ``d`` is a square symmetric matrix (the diagonal is ignored) or a condensed vector in the project's triangle order
    k = i (i - 1) / 2 + j, j < i; 2 <= n <= 16384; a NaN, an infinity, a cell whose mirror differs or a negative value is
    a ValueError that names the cell.  The values become int32 codes (``_capi.mantel_quantise``: the largest one lands in
    [2^30, 2^31), ``shift`` is reported) and the clustering is carried out on the codes in integers alone: pair sums in
    int64, averages compared by cross-multiplication in 128 bits, so no rounding decides a merge and tied averages are
    ties, broken towards the lower slots (include/suchtree_hip.h, st_linkage_codes, has the chain).  ``weights``: one
    integer >= 1 per object, total at most 65536 -- object i stands for that many coincident objects.  ``device``:
    None runs the host restatement, an index the kernels on that device -- the same integers; ... takes the host below
    LINKAGE_DEVICE_MIN objects and device 0 from there.  Returns a :class:`Dendrogram`.  WPGMA, Ward and neighbour joining
    are not exact in integers and are not offered.  An extension: the reference has no counterpart.
    """
    from . import _capi
    if method not in LINKAGE_METHODS:
        raise ValueError("method must be one of %s" % (LINKAGE_METHODS,))
    square = np.ndim(d) == 2
    v, n = mantel_condensed(d, "d", least=2)
    bad = np.flatnonzero(v < 0)
    if len(bad):
        k = int(bad[0])
        i = (1 + math.isqrt(8 * k + 1)) // 2
        where = "d[%d][%d]" % (i, k - i * (i - 1) // 2) if square else "d[%d]" % k
        raise ValueError("%s = %r is negative" % (where, float(v[k])))
    codes, shift = _capi.mantel_quantise(v)
    rows = _capi.linkage_codes(codes, weights, method, _linkage_device(device, n))
    return Dendrogram(n, method, shift, rows)


_linkage = linkage      # (dendrogram_congruence has an argument of that name)


class TopologyTestResult:
    """The topology test of phylosymbiosis (SuchTree.dendrogram_congruence, SuchLinkedTrees.phylosymbiosis_topology): is
    the dendrogram of a distance matrix closer to the tree than the dendrogram with its objects relabelled?

    Tree A of the match is the dendrogram, tree B the tree: ``rf``, ``rf_normalised``, ``exact``, ``n_a``, ``n_b`` and
    ``mean_transfer`` are those of :class:`CladeMatches` (``matches``, the observed one), ``transfer_total`` the integer
    sum of the transfer distances of the dendrogram's clades.  ``n_le`` counts the relabellings with rf_p <= rf,
    ``transfer_n_le`` those with transfer_total_p <= transfer_total -- integers against integers, a relabelling that maps
    the dendrogram onto itself ties and counts -- and ``p_value`` = (n_le + 1) / (permutations + 1), ``transfer_p_value``
    likewise.  ``perm_rf`` / ``perm_transfer`` (int64, in draw order) with ``keep_stats=True``, else None.
    ``dendrogram``, ``linkage``, ``rooted``, ``permutations``, ``seed``, ``stream`` repeat the run; ``leaves`` / ``names``
    / ``measure`` are filled in by the facades.  Unpacks as ``rf, p, n = result``.  These are this library's
    definitions: not claimed to reproduce another package's p-values.
    """

    def __init__(self, **kw):
        self.leaves = self.names = self.measure = None
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.rf, self.p_value, self.n))

    def __repr__(self):
        return "TopologyTestResult(rf=%d, p_value=%r, transfer_total=%d, transfer_p_value=%r, n=%d, linkage=%r, permutations=%d)" % (
            self.rf, self.p_value, self.transfer_total, self.transfer_p_value, self.n, self.linkage, self.permutations)


def _topology_counts(m, rooted, size_a, n_b, distance, match):
    """(rf, transfer_total) of one st_clade_match result, as CladeMatches defines them, in Python ints"""
    distance = distance.astype(np.int64)
    found = match >= 0
    p = size_a if rooted else np.minimum(size_a, m - size_a)
    transfer = np.where(found, np.minimum(distance, p - 1), p - 1)
    return len(size_a) + n_b - 2 * int((found & (distance == 0)).sum()), int(transfer.sum())


def dendrogram_congruence(flat, leaf_ids, y, linkage="average", rooted=True, min_branch=None, permutations=999, seed=None, stream=0,
                          keep_stats=False, device=..., match_device=...):
    """The topology test behind SuchTree.dendrogram_congruence: the dendrogram of ``y`` (:func:`linkage` with method
    ``linkage``; a :class:`Dendrogram` is taken as it is) against the flat tree ``flat`` over ``leaf_ids``, object k of y
    being listed leaf k.

    The observed match is ``match_clades(dendrogram, tree)`` with ``rooted`` and ``min_branch`` (``min_branch=0.0``
    leaves out, on both sides, the clades that exist only because a tie was broken: their branch is 0).  Relabelling
    p = 1 .. permutations is sigma_p = ``hommola_permutation(seed, stream, p, 0, n)``, numbered as :func:`mantel` numbers
    its permutations: object sigma_p[k] of the dendrogram is aligned with listed leaf k.  Both trees' clade ranges are
    computed once; a relabelling is one ``_capi.clade_match`` call with another alignment, so the first k relabellings
    are the same for any ``permutations`` >= k.  ``device``: None = everything on the host; an index = the linkage and
    the matches on that device; ... = the linkage as :func:`linkage` decides and the matches on ``match_device`` (... =
    device 0).  The same integers either way.  Returns a :class:`TopologyTestResult`.
    """
    from . import _capi
    from .suchtree import int_arg, seed_arg
    if linkage not in LINKAGE_METHODS:
        raise ValueError("linkage must be one of %s" % (LINKAGE_METHODS,))
    permutations, stream = int_arg("permutations", permutations, (1 << 31) - 1, "2^31 - 1"), int_arg("stream", stream, (1 << 31) - 1, "2^31 - 1")
    seed = seed_arg(seed)
    ids = np.ascontiguousarray(leaf_ids, dtype=np.int64)
    n = len(ids)
    if ids.ndim != 1 or n < 4 or n > _capi.LINKAGE_MAX_OBJECTS:
        raise ValueError("%d leaves: 4 to %d" % (n, _capi.LINKAGE_MAX_OBJECTS))
    if device is ...:
        dev = 0 if match_device is ... else -1 if match_device is None else int_arg("match_device", match_device)
        link_device = dev if dev >= 0 and n >= LINKAGE_DEVICE_MIN else None
    else:
        dev = -1 if device is None else int_arg("device", device)
        link_device = device
    dend = y if isinstance(y, Dendrogram) else _linkage(y, linkage, device=link_device)
    if dend.n != n:
        raise ValueError("y is over %d objects, not over the %d leaves" % (dend.n, n))
    rooted = bool(rooted)
    d_flat = dend.to_flat()
    d_ids = np.fromiter((d_flat.leaves[str(i)] for i in range(n)), dtype=np.int64, count=n)
    side_a = clade_side(d_flat, d_ids, rooted, min_branch)
    observed = match_clades(d_flat, d_ids, flat, ids, rooted, None, min_branch, None if dev < 0 else dev, side_a=side_a)
    side_b = clade_side(flat, ids, rooted, min_branch)
    where_b = np.empty(n, dtype=np.int32)
    where_b[side_b[0]] = np.arange(n, dtype=np.int32)
    size_a = (side_a[3] - side_a[2]).astype(np.int64)
    n_b = len(side_b[1])

    def counts(pos_b):
        distance, match, _ = _capi.clade_match(n, pos_b, side_a[2], side_a[3], side_b[2], side_b[3], rooted, dev)
        return _topology_counts(n, rooted, size_a, n_b, distance, match)
    rf0, transfer0 = counts(where_b[side_a[0]])
    perm_rf, perm_transfer = np.zeros(permutations, dtype=np.int64), np.zeros(permutations, dtype=np.int64)
    inverse = np.empty(n, dtype=np.int64)
    for p in range(1, permutations + 1):
        inverse[hommola_permutation(seed, stream, p, 0, n)] = np.arange(n)      # (listed leaf inverse[o] meets object o)
        perm_rf[p - 1], perm_transfer[p - 1] = counts(where_b[inverse[side_a[0]]])
    n_le, transfer_n_le = int((perm_rf <= rf0).sum()), int((perm_transfer <= transfer0).sum())
    return TopologyTestResult(rf=rf0, rf_normalised=observed.rf_normalised, exact=observed.exact, n_a=observed.n_a, n_b=observed.n_b,
                              transfer_total=transfer0, mean_transfer=observed.mean_transfer, n_le=n_le, transfer_n_le=transfer_n_le,
                              p_value=(n_le + 1) / (permutations + 1), transfer_p_value=(transfer_n_le + 1) / (permutations + 1),
                              perm_rf=perm_rf if keep_stats else None, perm_transfer=perm_transfer if keep_stats else None, matches=observed,
                              dendrogram=dend, linkage=dend.method, rooted=rooted, permutations=permutations, seed=seed, stream=stream, n=n)
