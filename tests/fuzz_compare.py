"""Seeded fuzz of the two-tree compare path under the rules of tests/fuzz_analyses.py (whose Census, case_rng, describe and
run this module uses with its own family tables).  Generators and checkers only: tests/test_fuzz_compare_host.py runs the
"host" layer (no GPU) and asserts the census of the device sessions; tests/test_gpu_fuzz_compare.py runs the "device" layer.

  family     entry                                        device layer: the GPU against                  host layer: that yardstick against
  moments    compare_{triangle,pairs}_host                compare_reference._Sums, np.histogram2d        numpy's moments, the searchsorted rule
  ranks      compare_{triangle,pairs}_ranks_host          rank_reference.rank_sums                       scipy's midranks, st_spearman_host
  kendall2   compare_{triangle,pairs}_kendall_host        kendall_reference.brute_counts                 st_kendall_host, scipy's kendalltau
  rows       compare_rows_host                            a row alone, elsewhere, another chunk; _Sums   (as moments, on one row)
  quartets   compare_quartets[_leaves]_host               the pick rule over MRCA ids walked in Python   the four-point rule, the oracle's sisters,
                                                                                                         the enumeration and draw in Python
  clades     compare_clades_host                          _Sums on each node's links; brute counts       st_clade_plan against clade_layout
  hommola    hommola_clades_host                          compare_rows_host on Layout.rows               st_hommola_permutation
  linked     SuchLinkedTrees: linklist, _links_in_order,  linked_distances_by_clade(tree=) and           a restatement from the dense matrix
             _partner_rows, the subset state              hommola_by_clade(tree=, max_leaves=) against a
                                                          second object's per-clade loop; and the host's

Every device case draws two trees on one device -- shape, node numbering, special branch lengths, strategy and handle
options -- two aligned id lists and the entry's own arguments together.  The yardstick of the float and integer families is
the per-pair distances of triangle_host / distances_host on the same two handles, held case by case to the CPU oracle's
bits (the drawn options sit under them).

The census is computed from the draws, from the oracle's distances of the drawn pairs and from the layout rules restated
below, never asked of the library -- with one exception: which quartets a call holds is taken from st_quartet_positions
on the host (device = -1, no GPU), which the host layer pins to the enumeration and the seeded draw of quartet_reference in
Python integers; 200,000 draws a case in Python integers would take minutes.  By hand:
  python tests/fuzz_compare.py FAMILY [cases] [seed] [host|device] [first case]"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import fuzz_analyses      # noqa: E402
import fuzz_parity      # noqa: E402
from compare_reference import SHIFT_PAIRS, _Sums, _check_shift, _rel      # noqa: E402
from fuzz_analyses import Census, _first_diff, case_rng, describe      # noqa: E402,F401
from oracle.oracle import OracleTree      # noqa: E402
from suchtree_amd import _capi, synth      # noqa: E402
from suchtree_amd.compare import DistanceComparison      # noqa: E402
from test_tables_emulated import _general_tree      # noqa: E402

FAMILIES = ("moments", "ranks", "kendall2", "rows", "quartets", "clades", "hommola", "linked")
INTEGER = ("ranks", "kendall2")      # infinities are ordinary values there: lengths that overflow float32 are drawn
TILE = _capi.CLADE_TILE              # ST_CLADE_TILE: chunk_pairs is a multiple of it
KTILE = _capi.KENDALL_TILE           # ST_KENDALL_TILE
CHUNK_PAIRS = 1 << 22                # host_compare.h: kCompareChunkPairs
CHUNK_CLADES = 1 << 25               # compare_plan.h: kCladeChunkPairs (the rows' default chunk)
ROWS_CHUNK_BLOCKS = 1 << 18          # compare_plan.h: kRowsChunkBlocks
LANE_PIECE = 64                      # kernels_clades.h: kCladeLanePiece
MAX_CELLS = 16384                    # kernels_compare.h: kCmpMaxCells
OPTS = dict(fuzz_parity.OPTS)        # (heap_lines, heap_codes and sort_tile are among them)
SKEWS = (0.0, 0.2, 0.5, 0.7, 0.8, 0.9, 0.97, 0.995)
ROW_M = (0, 1, 2, 11, 12, 91, 92, 129, 182)

# leaves: leaves per tree; m: ids per list; pairs: pairs of an explicit-pairs call; big: one pairs call in sixteen above
# kCompareChunkPairs (moments); kendall: pairs of a Kendall case (the reference looks at every pair of pairs); rows: rows;
# quartets: quartets of a call; clade_leaves: leaves of a clade tree; links: links of a clades call;
# universe: leaves of a tree of a Hommola call (one case in sixteen of `big`: 2,049 to 2,300 on one side)
LAYERS = {
    "host": {"device": -1, "leaves": 64, "m": 40, "pairs": 600, "big": False, "kendall": 700, "rows": 6, "quartets": 3000, "clade_leaves": 40, "links": 60, "universe": 100},
    "device": {"device": 0, "leaves": 3000, "m": 600, "pairs": 20000, "big": True, "kendall": TILE + 200, "rows": 300,
               "quartets": 200000, "clade_leaves": 400, "links": 600,
               "universe": 300},
}


# ---- the layout rules, restated (host_compare.h, compare_plan.cpp, kernels_rows.h) ----


def hist_in_lds(bins_x, bins_y):
    """MomentsReduce::start: uint32 counters ((cells + 1) & ~1) * 4 bytes, the edges beside them in LDS iff both fit 128 KiB"""
    return ((bins_x * bins_y + 1) & ~1) * 4 + (bins_x + bins_y + 2) * 8 <= 128 * 1024


def rows_layout(n_rows, m, chunk_pairs):
    """compare_plan.cpp: rows_layout -- (P, blocks per row, rows per chunk or None, dense)"""
    C = chunk_pairs if chunk_pairs > 0 else CHUNK_CLADES
    P = m * (m - 1) // 2
    if P == 0:
        return 0, 0, None, True
    nb = -(-P // TILE)
    if P <= C // 2:
        return P, nb, max(1, min(n_rows, C // P, ROWS_CHUNK_BLOCKS // nb)), True
    return P, nb, None, False


# ---- the shared draw: two trees on one device, two aligned id lists ----


def _leaf_count(rng, top):
    if rng.integers(3) == 0:
        k = int(rng.integers(1, int(math.log2(top)) + 1))
        return int(min(top, max(2, (1 << k) + int(rng.integers(-1, 2)))))
    return int(min(top, max(2, round(2.0 ** rng.uniform(1.0, math.log2(top))))))


def _tree(rng, L, family, shallow=False):
    """(parent, dist, tags) of one drawn tree.  shallow: balanced or nearly so (the oracle walks a pair's whole lineage)"""
    exact = L.get("leaves_exact")      # (a leaf count to be met: no balanced tree, whose leaves are a power of two)
    leaves = exact or max(L.get("leaves_lo", 2), _leaf_count(rng, L["leaves"]))
    kind = int(rng.integers(2, 8)) if exact else int(rng.integers(2 if shallow else 8))
    tags = []
    if kind < 2:
        parent, dist = synth.balanced_tree(int(min(12, max(1, round(math.log2(leaves))))), seed=int(rng.integers(1 << 31)))
        if kind == 0:      # every length equal: massive ties
            dist = np.where(parent < 0, np.float32(-1.0), np.float32((0.25, 1.0, 3.0)[int(rng.integers(3))])).astype(np.float32)
            tags.append("equal lengths")
        tags.append("balanced")
    elif kind == 2:
        parent, dist = synth.caterpillar_tree(min(leaves, 1500), seed=int(rng.integers(1 << 31)))
        tags.append("caterpillar")
    elif kind == 3:
        parent, dist = _general_tree(rng, 2 * leaves, int(rng.integers(2, 9)))
        tags.append("general")
    else:
        parent, dist = synth.skewed_tree(rng, leaves, float(rng.choice(SKEWS)))
        tags.append("skewed")
    parent, dist = np.asarray(parent, dtype=np.int32), np.asarray(dist, dtype=np.float32).copy()
    n = len(parent)
    if rng.integers(4) == 0:      # ids that are not in-order positions
        new_id = rng.permutation(n)
        p2, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
        p2[new_id] = np.where(parent >= 0, new_id[np.maximum(parent, 0)], -1)
        d2[new_id] = dist
        parent, dist = p2, d2
        tags.append("permuted ids")
    if rng.integers(4) == 0:      # special lengths on a tenth of the edges, one time in three on a half
        pool = [0.0, -0.5, 2.220446e-16] + ([3e37, 3e38] if family in INTEGER else [])      # (3e38: two edges overflow)
        k = rng.integers(0, n, max(1, n // (2 if rng.integers(3) == 0 else 10)))      # (a half: distances below zero)
        dist[k] = rng.choice(np.array(pool, np.float32), len(k))
        dist[parent < 0] = -1.0
        tags.append("special lengths")
    return parent, dist, tags


def _handle_draw(rng):
    strategy = str(rng.choice(["auto", "auto", "canopy", "walk"]))
    opts = {str(k): int(rng.choice(OPTS[str(k)])) for k in rng.choice(list(OPTS), int(rng.integers(0, 5)), replace=False)}
    return strategy, opts


def _leaves_of(parent):
    return np.flatnonzero(np.bincount(parent[parent >= 0], minlength=len(parent)) == 0).astype(np.int64)


def _ids(rng, parent, shape, any_node):
    """ids over the leaves (without repeats where the tree has enough), or -- any_node -- over every node with repeats"""
    if any_node:
        return rng.integers(0, len(parent), shape).astype(np.int64)
    leaves, count = _leaves_of(parent), int(np.prod(shape))
    if len(shape) == 1 and count <= len(leaves):
        return rng.choice(leaves, count, replace=False)
    return rng.choice(leaves, shape)


def _two_trees(rng, L, family, shallow=False, top_y=None, sizes=None):
    """top_y: tree y has 4 to top_y leaves (the clade tree: its every node is looked at); sizes: a layer per tree"""
    case = {"family": family}
    for s in "xy":
        Ls = dict(L, leaves=min(L["leaves"], top_y), leaves_lo=4) if top_y and s == "y" else sizes[s] if sizes else L
        case["parent_" + s], case["dist_" + s], tags = _tree(rng, Ls, family, shallow)
        case["shape_" + s] = "+".join(tags)
        case["strategy_" + s], case["opts_" + s] = _handle_draw(rng)
    case["same_tree"] = bool(rng.integers(12) == 0)      # tree_x == tree_y is allowed
    if case["same_tree"]:
        a, b = ("x", "y") if top_y or sizes else ("y", "x")
        for k in ("parent_", "dist_", "shape_", "strategy_", "opts_"):
            case[k + a] = case[k + b]
    case["any_node"] = bool(rng.integers(8) == 0)
    case["env"] = {}
    return case


def _handles(case):
    """the two DeviceTree handles of a case.  A strategy a tree's shape does not admit (canopy on a deep tree) falls back
    to auto, which case['refused'] and the census say; any other refusal -- a walk or auto handle, an option -- raises, and
    the session fails."""
    out, refused = [], []
    for s in "xy":
        if s == "y" and case["same_tree"]:
            out.append(out[0])
            break
        try:
            dev = _capi.DeviceTree(case["parent_" + s], case["dist_" + s], strategy=case["strategy_" + s])
        except Exception:      # noqa: BLE001
            if case["strategy_" + s] != "canopy":
                raise
            refused.append("canopy_" + s)
            dev = _capi.DeviceTree(case["parent_" + s], case["dist_" + s])
        for k, v in case["opts_" + s].items():
            dev.set_option(k, v)      # (every drawn value is in the option's range: a refusal is a failure)
        out.append(dev)
    case["refused"] = refused      # (printed in a mismatch line)
    if case.get("_census") is not None:
        case["_census"]["canopy refused by the shape, auto taken"] += len(refused)
    return out


def _pair_input(rng, case, L, top_pairs, counts=(), top_m=None):
    """Either a triangle range over m ids or explicit pairs drawn as indices into them; `counts`: pair counts to hit often"""
    any_node = case["any_node"]
    u = int(rng.integers(4))
    m = int((2, 3, 129, 182)[int(rng.integers(4))]) if u == 0 else int(round(2.0 ** rng.uniform(1.0, math.log2(L["m"]))))
    m = min(m, top_m or L["m"])
    case["m"] = m
    case["ids_x"], case["ids_y"] = _ids(rng, case["parent_x"], (m,), any_node), _ids(rng, case["parent_y"], (m,), any_node)
    case["entry"] = ("triangle", "pairs")[int(rng.integers(2))]
    v = int(rng.integers(8))
    if case["entry"] == "triangle":
        K = m * (m - 1) // 2
        want = int(rng.choice(counts)) if len(counts) and v >= 5 else None
        if want is not None and want <= min(K, top_pairs):
            count = want
            begin = int(rng.integers(0, K - count + 1))
        elif v < 2:
            begin, count = 0, K
        elif v == 2:
            count = min(K, int(rng.integers(0, 3)))
            begin = int(rng.integers(0, K - count + 1))
        else:
            begin = int(rng.integers(0, K + 1))
            count = int(rng.integers(0, K - begin + 1))
        if count > top_pairs:
            count = top_pairs
        case["k_begin"], case["k_count"] = begin, count
    else:
        if len(counts) and v >= 5:
            n = int(rng.choice(counts))
        elif v == 0:
            n = int(rng.integers(0, 3))
        else:
            n = int(round(2.0 ** rng.uniform(1.0, math.log2(top_pairs))))
        n = min(n, top_pairs)
        idx = rng.integers(0, m, (n, 2))
        case["repeated"] = bool(n > 8 and rng.integers(4) == 0)
        if case["repeated"]:
            idx = idx[rng.integers(0, n // 8, n)]
        case["idx"] = idx
    return case


def _pairs_of(case):
    """the call's pairs as explicit (n, 2) id arrays: pair k of the triangle is (ids[j], ids[i]), k = i (i - 1) / 2 + j"""
    if case["entry"] == "triangle":
        i, j = np.tril_indices(case["m"], -1)
        sel = slice(case["k_begin"], case["k_begin"] + case["k_count"])
        idx = np.stack((j[sel], i[sel]), axis=1)
    else:
        idx = case["idx"]
    return case["ids_x"][idx], case["ids_y"][idx]


def _threads():
    return min(16, len(os.sched_getaffinity(0)))


def _oracle(case, s, pairs):
    key = "_oracle_" + ("x" if case["same_tree"] else s)
    if key not in case:
        case[key] = OracleTree(case["parent_" + s], case["dist_" + s])
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    return case[key].distances_mt(pairs, max(1, min(_threads(), len(pairs) // 256))) if len(pairs) else np.zeros(0)


def columns(case):
    """the CPU oracle's distances of the call's pairs, (x, y) as float64: what the device's generated pairs must reduce"""
    if "_columns" not in case:
        px, py = _pairs_of(case)
        case["_columns"] = (_oracle(case, "x", px), _oracle(case, "y", py))
    return case["_columns"]


def _same_bits(got, want):
    return np.array_equal(np.nan_to_num(got, nan=-7.0).view(np.uint64), np.nan_to_num(want, nan=-7.0).view(np.uint64))


def _yardstick(case, dx, dy):
    """the call's per-pair distances from the two handles, after holding them to the oracle's bits"""
    if case["entry"] == "triangle":
        x, _ = dx.triangle_host(case["ids_x"], case["k_begin"], case["k_count"])
        y, _ = dy.triangle_host(case["ids_y"], case["k_begin"], case["k_count"])
    else:
        px, py = _pairs_of(case)
        x, _ = dx.distances_host(px)
        y, _ = dy.distances_host(py)
    x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)      # (copies: the library recycles result blocks)
    wx, wy = columns(case)
    if not (_same_bits(x, wx) and _same_bits(y, wy)):
        return None, None, "the handles' per-pair distances are not the oracle's bits (options %s / %s)" % (case["opts_x"], case["opts_y"])
    return x, y, None


def _call(case, dx, dy, suffix="", **kw):
    """the case's entry: compare_{triangle,pairs}{suffix}_host"""
    if case["entry"] == "triangle":
        return getattr(dx, "compare_triangle%s_host" % suffix)(dy, case["ids_x"], case["ids_y"], case["k_begin"], case["k_count"], **kw)
    px, py = _pairs_of(case)
    return getattr(dx, "compare_pairs%s_host" % suffix)(dy, px, py, **kw)


def _shared_census(case, C):
    for s in "xy":
        for tag in case["shape_" + s].split("+"):
            C["tree " + tag] += 1
        C["strategy " + case["strategy_" + s]] += 1
        C["handle options drawn"] += bool(case["opts_" + s])
    C["tree_x is tree_y"] += case["same_tree"]
    C["internal nodes and repeated ids"] += case["any_node"]


_SHARED = ["tree balanced", "tree equal lengths", "tree caterpillar", "tree general", "tree skewed", "tree permuted ids", "tree special lengths",
           "strategy auto", "strategy canopy", "strategy walk", "handle options drawn", "internal nodes and repeated ids"]


# ---- the float bars ----


def _empty_record(m):
    """an empty range: n = 0, zero sums, NaN min / max"""
    ok = m["n"] == 0 and all(m[k] == 0.0 for k in ("sx", "sy", "sxx", "syy", "sxy")) and all(
        math.isnan(m[k]) for k in ("min_x", "max_x", "min_y", "max_y"))
    return None if ok else "an empty range's record is not n = 0, zero sums, NaN min / max: %s" % (m,)


class _Record:
    """a st_pair_moments numpy row with the attributes of _capi.PairMoments"""

    def __init__(self, row):
        for k in _capi.PAIR_MOMENTS.names:
            setattr(self, k, row[k].item())


def _bars(m, x, y, edges=None, hist=None, shift_rule=_check_shift):
    """_Sums.check and the shift rule on one record over the columns x, y; a message, or None"""
    if len(x) == 0:
        bad = _empty_record({k: getattr(m, k) for k in _capi.PAIR_MOMENTS.names})
        return bad or (None if hist is None or not hist.any() else "an empty range's histogram is not zero")
    s = _Sums(m.shift_x, m.shift_y, edges)
    s.add(x, y)
    try:
        shift_rule(m, x, y)
    except AssertionError as e:
        return "shift: %s" % (e,)
    try:
        s.check(m, hist)
    except AssertionError as e:
        return "_Sums.check: %s" % (e.args[0] if e.args else "histogram",)
    return None


# ---- moments ----


def _moments_draw(rng, L):
    big = bool(L["big"] and rng.integers(16) == 0)
    case = _two_trees(rng, L, "moments", shallow=big)
    _pair_input(rng, case, L, L["pairs"], counts=(1, 2, SHIFT_PAIRS - 1, SHIFT_PAIRS + 1))
    if big:      # above kCompareChunkPairs: st_compare_pairs_host takes a second chunk
        case["entry"], case["repeated"] = "pairs", False
        case["idx"] = rng.integers(0, case["m"], (CHUNK_PAIRS + int(rng.integers(1, 5000)), 2))
    bx = int(rng.choice([1, 2, 127, 128]))
    by = int(rng.choice([1, 2, 127, 128, MAX_CELLS // bx]))
    if bx * by > MAX_CELLS:
        by = MAX_CELLS // bx
    case["bins"] = (bx, by) if rng.integers(5) else None
    case["edge_q"] = [float(v) for v in (rng.uniform(0.0, 0.15), rng.uniform(0.8, 1.0), rng.uniform(0.0, 0.15), rng.uniform(0.8, 1.0))]
    case["split"] = float(rng.random())
    return case


def _edges(case):
    """increasing edges over a drawn quantile range of the oracle's columns: the range clips the data"""
    if case["bins"] is None:
        return None
    x, y = columns(case)
    out = []
    for v, bins, (q0, q1) in ((x, case["bins"][0], case["edge_q"][:2]), (y, case["bins"][1], case["edge_q"][2:])):
        lo, hi = (np.quantile(v, [q0, q1]) if len(v) else (0.0, 1.0))
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            lo = lo if np.isfinite(lo) else 0.0
            hi = lo + 1.0
        out.append(np.linspace(lo, hi, bins + 1))
    return tuple(out)


def _moments_census(case, C):
    _shared_census(case, C)
    x, y = columns(case)
    n = len(x)
    for k in (0, 1, 2):
        C["n = %d" % k] += n == k
    C["fewer than 4096 pairs"] += 2 < n < SHIFT_PAIRS
    C["more than 4096 pairs"] += n > SHIFT_PAIRS
    C["entry " + case["entry"]] += 1
    if case["entry"] == "triangle" and case["k_count"]:
        i = int((1 + math.isqrt(1 + 8 * case["k_begin"])) // 2)      # the row of pair k_begin
        C["range begins in mid-row"] += case["k_begin"] != i * (i - 1) // 2
    C["a second chunk of pairs"] += case["entry"] == "pairs" and n > CHUNK_PAIRS
    edges = _edges(case)
    C["no histogram"] += edges is None
    if edges is not None:
        C["edges in LDS" if hist_in_lds(*case["bins"]) else "edges in global memory"] += 1
        if n:
            C["values outside the edges"] += bool(((x < edges[0][0]) | (x > edges[0][-1]) | (y < edges[1][0]) | (y > edges[1][-1])).any())
    if n >= 2:
        C["a constant column (r is NaN)"] += bool(x.min() == x.max() or y.min() == y.max())


def _merge_check(case, dx, dy, whole, hist, edges):
    """a call split at a drawn k and merged equals the whole call: n, histogram, min and max exactly, the derived values
    under 1e-12 relative as the merge test of test_gpu_reductions.py asks; a case that misses that bar is held to a bound
    derived below, and counted"""
    px, py = _pairs_of(case)
    n = len(px)
    cut = int(case["split"] * (n + 1))
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        if case["entry"] == "triangle":
            m, h = dx.compare_triangle_host(dy, case["ids_x"], case["ids_y"], case["k_begin"] + lo, hi - lo, edges=edges)
        else:
            m, h = dx.compare_pairs_host(dy, px[lo:hi], py[lo:hi], edges=edges)
        parts.append(DistanceComparison.from_moments(m, h, *(edges or (None, None))))
    merged = DistanceComparison.merge(*parts)
    full = DistanceComparison.from_moments(whole, hist, *(edges or (None, None)))
    if merged.n_pairs != n or (edges is not None and not np.array_equal(merged.hist, full.hist)):
        return "split at %d and merged: n or the histogram differ" % cut
    if n == 0:
        return None
    for k in ("min_x", "max_x", "min_y", "max_y"):
        if getattr(merged, k) != getattr(full, k):
            return "split at %d and merged: %s %r against %r" % (cut, k, getattr(merged, k), getattr(full, k))
    bad, derived = _merge_bars(merged, full, n)
    if bad:
        return "split at %d and merged: %s" % (cut, bad)
    if derived and case.get("_census") is not None:
        case["_census"]["merge: the bound derived from the raw moment about the shift, for " + ", ".join(derived)] += 1
    return None


def _merge_bars(merged, full, n):
    """(a message or None, the keys that needed the derived bound) for the derived values of a merged result against the
    whole call's: the _rel < 1e-12 of the existing merge test first, as it stands (tests/test_fuzz_compare_host.py pins
    the fallback on a constructed column)."""
    keys = ("mean_x", "mean_y", "var_x", "var_y", "cov", "pearson_r")
    strict = [k for k in keys if not ((math.isnan(getattr(merged, k)) and math.isnan(getattr(full, k)))
                                      or _rel(getattr(merged, k), getattr(full, k)) < 1e-12)]
    if not strict:
        return None, []
    # Only where that bar is missed: the merged and the whole record are two roundings of the same sums about a shift, so
    # they differ by that rounding -- a few ulps of the raw moment about the shift, msx = sxx / n, not of the variance
    # msx - (sx / n)^2, which in a nearly constant column is smaller by orders of magnitude.  The same 1e-12 is therefore
    # taken of the raw moment (of its root for a mean); r inherits dcov / sqrt(vx vy) + |r| (dvx / 2 vx + dvy / 2 vy), and
    # where a variance lies within its bound of zero r is NaN or anything.
    msx, msy = full.sxx / n, full.syy / n
    scale = {"mean_x": math.sqrt(msx), "mean_y": math.sqrt(msy), "var_x": msx, "var_y": msy, "cov": math.sqrt(msx * msy)}
    for k in strict:
        g, w = getattr(merged, k), getattr(full, k)
        if k != "pearson_r":
            ok = abs(g - w) <= 1e-12 * scale[k]
        elif min(full.var_x, merged.var_x) <= 1e-12 * msx or min(full.var_y, merged.var_y) <= 1e-12 * msy:
            ok = True
        else:
            ok = not (math.isnan(g) or math.isnan(w)) and abs(g - w) <= 1e-12 * (
                math.sqrt(msx * msy / (full.var_x * full.var_y)) + abs(w) * (msx / (2 * full.var_x) + msy / (2 * full.var_y)))
        if not ok:
            return "%s %r against %r (the bar of the merge test and the bound derived from the raw moment)" % (k, g, w), strict
    return None, strict


def _moments_check(case, rng, L):
    x, y = columns(case)
    edges = _edges(case)
    if L["device"] < 0:
        return _moments_host(case, x, y, edges)
    dx, dy = _handles(case)
    x, y, bad = _yardstick(case, dx, dy)
    if bad:
        return bad
    m0, none = _call(case, dx, dy)
    if none is not None:
        return "a histogram came back though none was asked for"
    mh, hist = _call(case, dx, dy, edges=edges) if edges is not None else (m0, None)
    if bytes(mh) != bytes(m0):
        return "the histogram changed the moments: %s against %s" % (mh.as_dict(), m0.as_dict())
    return _bars(m0, x, y, edges, hist) or _merge_check(case, dx, dy, m0, hist, edges)


def _moments_host(case, x, y, edges):
    """the reference alone, on the oracle's columns: _Sums about the shift rule's shift against np.mean, np.var, np.cov,
    np.corrcoef under the project's bars, its histogram against a searchsorted count"""
    if len(x) == 0:
        return None
    cx, cy = x[:SHIFT_PAIRS].mean(), y[:SHIFT_PAIRS].mean()
    s = _Sums(cx, cy, edges)
    s.add(x, y)
    c = DistanceComparison.from_sums(s.n, cx, cy, s.sx, s.sy, s.sxx, s.syy, s.sxy, s.min_x, s.max_x, s.min_y, s.max_y)
    for got, want, what in ((c.mean_x, x.mean(), "mean_x"), (c.mean_y, y.mean(), "mean_y"), (c.var_x, np.var(x), "var_x"),
                            (c.var_y, np.var(y), "var_y"), (c.cov, np.cov(x, y, bias=True)[0, 1] if len(x) > 1 else 0.0, "cov")):
        if not (_rel(got, want) < 1e-10 or abs(got - want) < 1e-12):
            return "reference %s %r, numpy's %r" % (what, got, want)
    if np.var(x) > 0 and np.var(y) > 0 and c.var_x > 0 and c.var_y > 0:
        if not abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-10:
            return "reference r %r, np.corrcoef's %r" % (c.pearson_r, np.corrcoef(x, y)[0, 1])
    if edges is not None:      # the contract's rule: searchsorted side='right' - 1, the last edge in the last bin
        cell = []
        for v, e in ((x, edges[0]), (y, edges[1])):
            b = np.searchsorted(e, v, side="right") - 1
            b[v == e[-1]] = len(e) - 2
            cell.append(np.where((v >= e[0]) & (v <= e[-1]), b, -1))
        keep = (cell[0] >= 0) & (cell[1] >= 0)
        want = np.zeros(s.hist.shape, np.int64)
        np.add.at(want, (cell[0][keep], cell[1][keep]), 1)
        if not np.array_equal(s.hist, want):
            return "np.histogram2d differs from the searchsorted rule of the contract"
    return None


# ---- ranks and kendall2 ----


def _chunks_draw(rng, case, n_values=3):
    """three of: 0, 8192, 16384, one tile above the pair count"""
    n = _n_pairs(case)
    pool = [0, TILE, 2 * TILE, (n // TILE + 1) * TILE]
    return [int(v) for v in rng.permutation(pool)[:n_values]]


def _n_pairs(case):
    return case["k_count"] if case["entry"] == "triangle" else len(case["idx"])


def _stat_draw(rng, L, family):
    case = _two_trees(rng, L, family)
    if family == "kendall2":
        _pair_input(rng, case, L, L["kendall"], counts=(1, KTILE - 1, KTILE, KTILE + 1, TILE + 64),
                    top_m=min(L["m"], 140))      # (m = 129: 8,256 pairs; the reference looks at every pair of pairs)
    else:
        _pair_input(rng, case, L, L["pairs"], counts=(1, 2, TILE + 64, TILE + 64, 2 * TILE + 1))
    case["chunks"] = _chunks_draw(rng, case)
    return case


def _stat_census(case, C):
    _shared_census(case, C)
    x, y = columns(case)
    n = len(x)
    C["n = 0"] += n == 0
    C["n = 1"] += n == 1
    C["entry " + case["entry"]] += 1
    small = [c for c in case["chunks"] if 0 < c < n]
    C["two chunks"] += bool(small)
    C["a sub-range that splits a chunk"] += case["entry"] == "triangle" and any(case["k_begin"] % c for c in small)
    C["repeated pairs"] += case["entry"] == "pairs" and case["repeated"]
    nan = bool(n and (np.isnan(x) | np.isnan(y)).any())
    C["a NaN"] += nan
    C["an infinity"] += bool(n and (np.isinf(x) | np.isinf(y)).any())
    if n and not nan:
        import rank_reference
        groups = [int(np.unique(v, return_counts=True)[1].max()) for v in (x, y)]
        buckets = [len(rank_reference.buckets_of(v.astype(np.float32))) for v in (x, y)]
        C["one occupied bucket"] += min(buckets) == 1
        C["several buckets"] += max(buckets) > 1
        C["a tie group of all pairs"] += n > 1 and max(groups) == n
        C["a tie group wider than a tile"] += max(groups) > KTILE
        C["negative and positive values in one column"] += any((v < 0).any() and (v > 0).any() for v in (x, y))
        C["a zero distance"] += bool((x == 0).any() or (y == 0).any())
        C["-0.0 and +0.0 in one column"] += any((np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any() for v in (x, y))
    for k, name in ((KTILE - 1, "one tile less one"), (KTILE, "one tile"), (KTILE + 1, "one tile and one")):
        C[name] += n == k


def _rank_tuple(r):
    return (int(r.n), int(r.n_nan), r.sxy, r.sxx, r.syy, int(r.distinct_x), int(r.distinct_y))


def _stat_check(case, rng, L, family):
    import kendall_reference
    import rank_reference
    x, y = columns(case)
    if family == "ranks":
        want = tuple(rank_reference.rank_sums(x, y))
    else:
        want = tuple(kendall_reference.brute_counts(x, y))
    if L["device"] < 0:
        return _stat_host(family, x.astype(np.float32), y.astype(np.float32), want)
    dx, dy = _handles(case)
    x, y, bad = _yardstick(case, dx, dy)
    if bad:
        return bad
    m0, _ = _call(case, dx, dy)
    first = None
    for chunk in case["chunks"]:
        m, second = _call(case, dx, dy, "_ranks" if family == "ranks" else "_kendall", chunk_pairs=chunk)
        if bytes(m) != bytes(m0):
            return "chunk_pairs %d: the moments are not the moments entry's bytes" % chunk
        got = _rank_tuple(second) if family == "ranks" else second.as_tuple()
        if got != want:
            return "chunk_pairs %d: got %s want %s" % (chunk, got, want)
        first = bytes(second) if first is None else first
        if bytes(second) != first:
            return "chunk_pairs %d: other bytes than chunk_pairs %d" % (chunk, case["chunks"][0])
    return None


def _stat_host(family, x, y, want):
    """the references against independent definitions on the oracle's columns"""
    import kendall_reference
    import rank_reference
    n = len(x)
    nan = bool((np.isnan(x) | np.isnan(y)).any())
    if family == "ranks":
        r = _capi.spearman_host(x, y)
        if _rank_tuple(r) != want:
            return "rank_sums %s, st_spearman_host %s" % (want, _rank_tuple(r))
        if n and not nan:
            theirs = rank_reference.scipy_midrank_sums(x, y)
            if theirs != want[2:5]:
                return "rank_sums %s, scipy's midranks give %s" % (want[2:5], theirs)
        return None
    k = _capi.kendall_host(x, y)
    if k.as_tuple() != want:
        return "brute_counts %s, st_kendall_host %s" % (want, k.as_tuple())
    mine = kendall_reference.tau_b(kendall_reference.KendallRef(*want))
    if n >= 2 and not nan and not math.isnan(mine):
        import scipy.stats
        theirs = float(scipy.stats.kendalltau(x, y).statistic)
        if not abs(mine - theirs) <= 1e-12:
            return "tau-b from the counts %r, scipy's %r" % (mine, theirs)
    return None


# ---- rows ----


def _rows_draw(rng, L):
    case = _two_trees(rng, L, "rows")
    u = int(rng.integers(4))
    n_rows = int((1, 2, L["rows"])[int(rng.integers(3))]) if u == 0 else int(round(2.0 ** rng.uniform(0.0, math.log2(L["rows"]))))
    m = int(rng.choice(ROW_M if L["device"] >= 0 else ROW_M[:5]))
    case["n_rows"], case["m"] = n_rows, m
    case["ids_x"] = _ids(rng, case["parent_x"], (n_rows, m), case["any_node"])
    case["ids_y"] = _ids(rng, case["parent_y"], (n_rows, m), case["any_node"])
    case["chunks"] = [int(v) for v in rng.permutation([0, TILE, 2 * TILE])[:2]]
    case["alone"] = [int(v) for v in rng.integers(0, n_rows, min(n_rows, 3))]
    case["order"] = rng.permutation(n_rows)
    return case


def _rows_census(case, C):
    _shared_census(case, C)
    n_rows, m = case["n_rows"], case["m"]
    C["m below 2"] += m < 2
    for chunk in case["chunks"]:
        P, nb, per_chunk, dense = rows_layout(n_rows, m, chunk)
        if P == 0:
            continue
        C["rows of at most 64 pairs (lane form)"] += P <= LANE_PIECE
        C["rows just above 64 pairs (m = 12)"] += m == 12
        C["dense layout"] += dense
        C["padded layout"] += not dense
        C["a short last block summed by lane 0"] += P > LANE_PIECE and P - (nb - 1) * TILE <= LANE_PIECE
        C["several blocks a row"] += nb > 1
        C["more rows than a chunk holds"] += dense and per_chunk < n_rows
    C["one row"] += n_rows == 1


def _row_shift(m, x, y):
    """a row's shift: its first pair, 0 where that is not finite"""
    for got, v in ((m.shift_x, x[0]), (m.shift_y, y[0])):
        assert got == (v if np.isfinite(v) else 0.0), (got, v)


def _rows_check(case, rng, L):
    X, Y = case["ids_x"], case["ids_y"]
    i, j = np.tril_indices(case["m"], -1)
    if L["device"] < 0:      # the reference alone on one row of the oracle's distances
        r = case["alone"][0]
        x = _oracle(case, "x", np.stack((X[r][j], X[r][i]), axis=1))
        y = _oracle(case, "y", np.stack((Y[r][j], Y[r][i]), axis=1))
        return _moments_host(case, x, y, None)
    dx, dy = _handles(case)
    out = dx.compare_rows_host(dy, X, Y, case["chunks"][0])
    bad = _first_diff(dx.compare_rows_host(dy, X, Y, case["chunks"][1]), out, "chunk_pairs %d against %d, row" % (case["chunks"][1], case["chunks"][0]))
    if bad:
        return bad
    order = case["order"]
    bad = _first_diff(dx.compare_rows_host(dy, X[order], Y[order], case["chunks"][0]), out[order], "the rows in another order, row")
    if bad:
        return bad
    for r in case["alone"]:
        bad = _first_diff(dx.compare_rows_host(dy, X[r:r + 1], Y[r:r + 1], case["chunks"][1]), out[r:r + 1], "row %d standing alone" % r)
        if bad:
            return bad
        x, _ = dx.triangle_host(X[r])
        y, _ = dy.triangle_host(Y[r])
        x, y = np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)
        wx = _oracle(case, "x", np.stack((X[r][j], X[r][i]), axis=1))
        wy = _oracle(case, "y", np.stack((Y[r][j], Y[r][i]), axis=1))
        if not (_same_bits(x, wx) and _same_bits(y, wy)):
            return "row %d: the handles' per-pair distances are not the oracle's bits" % r
        bad = _bars(_Record(out[r]), x, y, shift_rule=_row_shift)
        if bad:
            return "row %d: %s" % (r, bad)
    if case["m"] < 2:
        for r in range(case["n_rows"]):
            bad = _empty_record(out[r])
            if bad:
                return "row %d: %s" % (r, bad)
        return None
    # every row's record under the float bars, over the handles' distances of all the rows' pairs in one call a tree (the
    # rows above were also held to the oracle's bits)
    P = len(i)
    ax, _ = dx.distances_host(np.stack((X[:, j], X[:, i]), axis=2).reshape(-1, 2))
    ay, _ = dy.distances_host(np.stack((Y[:, j], Y[:, i]), axis=2).reshape(-1, 2))
    ax, ay = np.array(ax, dtype=np.float64).reshape(-1, P), np.array(ay, dtype=np.float64).reshape(-1, P)
    for r in range(case["n_rows"]):
        bad = _bars(_Record(out[r]), ax[r], ay[r], shift_rule=_row_shift)
        if bad:
            return "row %d: %s" % (r, bad)
    return None


# ---- quartets ----


def _quartets_draw(rng, L):
    case = _two_trees(rng, L, "quartets")
    m = 4 if rng.integers(6) == 0 else int(round(2.0 ** rng.uniform(2.0, 6.0)))
    case["m"] = m
    case["repeated"] = bool(rng.integers(8) == 0)      # ids drawn with repeats: class 3
    for s in "xy":
        pool = np.arange(len(case["parent_" + s])) if case["any_node"] else _leaves_of(case["parent_" + s])
        case["ids_" + s] = rng.choice(pool, m, replace=case["repeated"] or m > len(pool)).astype(np.int64)
    case["entry"] = ("all", "sample", "explicit")[int(rng.integers(3))]
    top = L["quartets"]
    if case["entry"] == "all":
        begin, count = fuzz_analyses._range(rng, math.comb(m, 4))
    elif case["entry"] == "sample":
        case["seed"] = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        begin = 0 if rng.integers(2) else int(rng.integers(0, 1 << int(rng.integers(1, 41))))
        count = int(rng.integers(0, 3)) if rng.integers(6) == 0 else int(round(2.0 ** rng.uniform(0.0, math.log2(top))))
    else:
        begin, count = 0, (int(rng.integers(0, 3)) if rng.integers(6) == 0 else int(round(2.0 ** rng.uniform(0.0, math.log2(top)))))
        case["pos"] = rng.integers(0, m, (count, 4))      # (a position may repeat within a row: class 3)
    count = min(count, top)
    case["k_begin"], case["k_count"] = begin, count
    chunks = [0, 1, 64, 257, count + 1]
    case["chunks"] = []
    for c in rng.permutation(chunks)[:2]:
        c = int(c)
        while c > 0 and count // c > 200:      # (a chunk is a launch: at most 200 of them, as fuzz_analyses coarsens its cuts)
            c *= 2
        case["chunks"].append(c)
    case["split"] = float(rng.random())
    return case


def _positions(case, begin=None, count=None):
    """the (count, 4) positions of the call's quartets: st_quartet_positions on the host, or the drawn rows"""
    begin = case["k_begin"] if begin is None else begin
    count = case["k_count"] if count is None else count
    if case["entry"] == "explicit":
        return case["pos"][begin: begin + count]
    return _capi.quartet_positions(case["entry"], case.get("seed", 0), case["m"], begin, count, device=-1).astype(np.int64)


def pick_classes(parent, ids, pos):
    """The contract's class of every row of positions: the six MRCA ids in the order ab ac ad bc bd cd, `pick` the first
    whose id occurs once among the six; 0 = ab|cd (pick 0 or 5), 1 = ac|bd (1 or 4), 2 = ad|bc (2 or 3), 3 = none unique.
    The MRCA ids by walking parents (quartet_reference.mrca_matrices)."""
    import quartet_reference
    M = quartet_reference.mrca_matrices(parent, ids)[1]
    a, b, c, d = np.asarray(pos, dtype=np.int64).reshape(-1, 4).T
    six = np.stack([M[a, b], M[a, c], M[a, d], M[b, c], M[b, d], M[c, d]], axis=1)
    once = (six[:, :, None] == six[:, None, :]).sum(axis=2) == 1
    pick = np.where(once.any(axis=1), once.argmax(axis=1), 6)
    return np.array([0, 1, 2, 2, 1, 0, 3])[pick]


def _classes(case, pos):
    return pick_classes(case["parent_x"], case["ids_x"], pos), pick_classes(case["parent_y"], case["ids_y"], pos)


def _quartets_census(case, C):
    _shared_census(case, C)
    count = case["k_count"]
    cx, cy = _classes(case, _positions(case))
    case["_classes"] = (cx, cy)
    C["class 3 present"] += bool((cx == 3).any() or (cy == 3).any())
    C["every class of distinct leaves present"] += all((cx == k).any() for k in range(3))
    C["a polytomy side"] += any(np.bincount(case["parent_" + s][case["parent_" + s] >= 0]).max() > 2 for s in "xy")
    C["m = 4"] += case["m"] == 4
    C["entry " + case["entry"]] += 1
    C["a range that begins past 0"] += case["entry"] != "explicit" and case["k_begin"] > 0 and count > 0
    C["several chunks"] += any(0 < c < count for c in case["chunks"])
    C["an empty range"] += count == 0


def _quartets_call(case, dx, dy, begin, count, chunk):
    if case["entry"] == "explicit":
        pos = case["pos"][begin: begin + count]
        return dx.compare_quartets_host(dy, case["ids_x"][pos], case["ids_y"][pos], chunk_quartets=chunk)
    return dx.compare_quartets_leaves_host(dy, case["ids_x"], case["ids_y"], case["entry"], case.get("seed", 0), begin, count, chunk)


def _quartets_check(case, rng, L):
    import quartet_reference as qr
    cx, cy = case["_classes"]
    begin, count = case["k_begin"], case["k_count"]
    if L["device"] < 0:
        return _quartets_host(case, cx, cy)
    dx, dy = _handles(case)
    want = qr.table_of(cx, cy)
    for chunk in case["chunks"]:
        got = _quartets_call(case, dx, dy, begin, count, chunk)
        if not np.array_equal(got, want):
            return "chunk_quartets %d: got %s want %s" % (chunk, got.tolist(), want.tolist())
    cut = int(case["split"] * (count + 1))
    lo = _quartets_call(case, dx, dy, begin, cut, case["chunks"][0])
    hi = _quartets_call(case, dx, dy, begin + cut, count - cut, case["chunks"][1])
    if not (np.array_equal(lo, qr.table_of(cx[:cut], cy[:cut])) and np.array_equal(lo + hi, want)):
        return "split at %d: %s + %s against %s" % (cut, lo.tolist(), hi.tolist(), want.tolist())
    return None


def _quartets_host(case, cx, cy):
    """the yardstick against independent definitions: the positions of st_quartet_positions on the host against the
    colexicographic enumeration and the seeded draw in Python integers; the pick rule over MRCA ids against the four-point
    rule over MRCA depths on rows of four distinct leaves, and against the sister pairs the CPU oracle reports"""
    import quartet_reference as qr
    pos = _positions(case)
    begin, m = case["k_begin"], case["m"]
    if case["entry"] == "all":
        if not np.array_equal(pos, qr.colex_quartets(m)[begin: begin + len(pos)]):
            return "st_quartet_positions (all) differs from the colexicographic enumeration"
        if len(pos) and list(pos[-1]) != qr.unrank_exact(begin + len(pos) - 1):
            return "st_quartet_positions (all) differs from unrank_exact at the last quartet"
    elif case["entry"] == "sample":
        for k in range(min(len(pos), 8)):
            if list(pos[k]) != qr.py_draw(case["seed"], begin + k, m):
                return "st_quartet_positions (sample) differs from py_draw at quartet %d" % (begin + k)
    for s, mine in (("x", cx), ("y", cy)):
        parent, ids = case["parent_" + s], case["ids_" + s]
        rows = ids[pos]
        if not case["any_node"]:
            distinct = (np.sort(rows, axis=1)[:, 1:] != np.sort(rows, axis=1)[:, :-1]).all(axis=1)
            four = qr.leaf_classes(parent, ids, pos[distinct])
            if not np.array_equal(mine[distinct], four):
                return "tree %s: the pick rule over MRCA ids differs from the four-point rule on distinct leaves" % s
            if (mine[distinct] == 3).any() and np.bincount(parent[parent >= 0]).max() <= 2:
                return "tree %s: class 3 on four distinct leaves of a binary tree" % s
        topo = _oracle_tree(case, s).quartets(rows)      # (0,1) and (2,3) are the sister pairs; class 3 reported as ab|cd
        sister = {0: (0, 1), 1: (0, 2), 2: (0, 3), 3: (0, 1)}
        for k in range(len(rows)):
            a, b = (int(rows[k][j]) for j in sister[int(mine[k])])
            halves = ({int(topo[k][0]), int(topo[k][1])}, {int(topo[k][2]), int(topo[k][3])})
            if {a, b} not in halves:
                return "tree %s quartet %d: class %d, the oracle's sisters %s" % (s, k, mine[k], topo[k].tolist())
    return None


def _oracle_tree(case, s):
    key = "_oracle_" + ("x" if case["same_tree"] else s)
    if key not in case:
        case[key] = OracleTree(case["parent_" + s], case["dist_" + s])
    return case[key]


# ---- clades ----


def clade_layout(parent, link_leaf, cap):
    """compare_plan.cpp: clade_plan restated -- (count per node, the link ranks under each node in rank order, the
    segments [(first_pair, n_pairs, kind, node)] in pair order).  Children in increasing id order; leaves take consecutive
    position ranges in preorder; the nodes within the cap emit their segments in the order of their link counts (ties:
    reverse preorder): a triangle for a leaf with two links and more, for an inner node a rectangle between each child's
    links and the links of its later children."""
    n = len(parent)
    kids = [[] for _ in range(n)]
    for v in range(n):
        if parent[v] >= 0:
            kids[parent[v]].append(v)
    pre, stack = [], [int(np.flatnonzero(parent < 0)[0])]
    while stack:
        v = stack.pop()
        pre.append(v)
        stack.extend(reversed(kids[v]))
    ranks = [[] for _ in range(n)]
    for j, leaf in enumerate(link_leaf.tolist()):
        ranks[leaf].append(j)
    begin, pos = [0] * n, 0
    for v in pre:
        if not kids[v]:
            begin[v] = pos
            pos += len(ranks[v])
    for v in reversed(pre):
        if kids[v]:
            ranks[v] = sorted(j for c in kids[v] for j in ranks[c])
            begin[v] = begin[kids[v][0]]
    count = [len(r) for r in ranks]
    segs, total = [], 0
    for v in sorted(reversed(pre), key=lambda u: count[u]):      # (sorted is stable)
        if cap is not None and count[v] > cap:
            continue
        end = begin[v] + count[v]
        if not kids[v]:
            if count[v] >= 2:
                segs.append((total, count[v] * (count[v] - 1) // 2, 1, v))
                total += segs[-1][1]
            continue
        for c in kids[v][:-1]:
            c0 = begin[c] + count[c]
            if count[c] > 0 and end > c0:
                segs.append((total, count[c] * (end - c0), 0, v))
                total += segs[-1][1]
    return np.array(count, dtype=np.int64), ranks, segs


def _pieces(segs):
    """the tile-sized pieces of the segments: a segment is cut where a tile of ST_CLADE_TILE pairs ends"""
    out = []
    for first, np_, _, _ in segs:
        k = first
        while k < first + np_:
            nxt = min(first + np_, (k // TILE + 1) * TILE)
            out.append(nxt - k)
            k = nxt
    return out


def _clades_draw(rng, L):
    case = _two_trees(rng, L, "clades", top_y=L["clade_leaves"])
    n_links = 0 if rng.integers(12) == 0 else int(round(2.0 ** rng.uniform(0.0, math.log2(L["links"]))))
    leaves_y = _leaves_of(case["parent_y"])
    pool = rng.choice(leaves_y, max(1, int(len(leaves_y) * rng.uniform(0.05, 1.0))), replace=False)      # (leaves without links)
    case["m"] = n_links
    case["ids_y"] = rng.choice(pool, n_links).astype(np.int64)      # (several links on one leaf)
    case["ids_x"] = _ids(rng, case["parent_x"], (n_links, 1), case["any_node"]).reshape(-1)
    case["cap"] = (None, 0, int(rng.integers(1, n_links + 2)))[int(rng.integers(3))]
    case["chunks"] = [int(v) for v in rng.permutation([0, TILE, 2 * TILE])[:2]]
    case["entry"], case["k_begin"], case["k_count"] = "triangle", 0, n_links * (n_links - 1) // 2      # (the yardstick: every pair of links)
    case["_layout"] = clade_layout(case["parent_y"], case["ids_y"], case["cap"])
    count = case["_layout"][0]
    live = np.flatnonzero((count >= 2) & (count <= (case["cap"] if case["cap"] is not None else n_links)))
    case["nodes"] = live      # every node with two links and more within the cap is held to the float bars
    return case


def _clades_census(case, C):
    _shared_census(case, C)
    count, _, segs = case["_layout"]
    pieces = _pieces(segs)
    total = sum(s[1] for s in segs)
    C["a piece of at most 64 pairs"] += any(p <= LANE_PIECE for p in pieces)
    C["a piece above 64 pairs"] += any(p > LANE_PIECE for p in pieces)
    C["a segment cut by a tile boundary"] += any(f // TILE != (f + n - 1) // TILE for f, n, _, _ in segs)
    C["two chunks"] += any(0 < c < total for c in case["chunks"])
    C["a triangle segment (several links on one leaf)"] += any(k == 1 for _, _, k, _ in segs)
    C["a node over the cap"] += case["cap"] is not None and bool((count > case["cap"]).any())
    C["no cap"] += case["cap"] is None
    C["no links"] += case["m"] == 0
    C["a caterpillar clade tree"] += "caterpillar" in case["shape_y"]
    C["a polytomy in the clade tree"] += int(np.bincount(case["parent_y"][case["parent_y"] >= 0]).max()) > 2
    C["a leaf without links inside a clade with links"] += bool(case["m"]) and len(np.unique(case["ids_y"])) < len(_leaves_of(case["parent_y"]))


def _no_shift_rule(m, x, y):
    """(a node's shift is whatever its first piece took: the sums are checked about the shift the record states)"""


def _clades_check(case, rng, L):
    count, ranks, segs = case["_layout"]
    parent, cap = case["parent_y"], case["cap"]
    if L["device"] < 0:      # the restated layout against st_clade_plan, the counts against a walk from every link to the root
        plan = _capi.clade_plan(parent, case["ids_y"], cap)
        walk = np.zeros(len(parent), dtype=np.int64)
        for leaf in case["ids_y"].tolist():
            v = leaf
            while v >= 0:
                walk[v] += 1
                v = int(parent[v])
        if not (np.array_equal(plan["count"], count) and np.array_equal(walk, count)):
            return "links under each node: the restatement, st_clade_plan and the walk to the root differ"
        got = [(int(g["first_pair"]), int(g["n_pairs"]), int(g["kind"]), int(g["node"])) for g in plan["segments"]]
        if got != segs or plan["total_pairs"] != sum(s[1] for s in segs):
            return "the restated segments differ from st_clade_plan's"
        for v in case["nodes"].tolist():
            if sorted(plan["perm"][plan["begin"][v]: plan["begin"][v] + plan["count"][v]].tolist()) != ranks[v]:
                return "node %d: the restated link ranks differ from st_clade_plan's" % v
        return None
    dx, dy = _handles(case)
    x, y, bad = _yardstick(case, dx, dy)
    if bad:
        return bad
    out, got_count = dx.compare_clades_host(dy, parent, case["ids_x"], case["ids_y"], cap, case["chunks"][0])
    other, _ = dx.compare_clades_host(dy, parent, case["ids_x"], case["ids_y"], cap, case["chunks"][1])
    bad = _first_diff(other, out, "chunk_pairs %d against %d, node" % (case["chunks"][1], case["chunks"][0]))
    if bad:
        return bad
    if not np.array_equal(got_count, count):
        return "links under each node: got %s want %s" % (got_count.tolist()[:20], count.tolist()[:20])
    over = count > cap if cap is not None else np.zeros(len(count), dtype=bool)
    want_n = np.where(over, -1, count * (count - 1) // 2)
    if not np.array_equal(out["n"], want_n):
        v = int(np.flatnonzero(out["n"] != want_n)[0])
        return "node %d with %d links under cap %s: n %d want %d" % (v, count[v], cap, out["n"][v], want_n[v])
    for v in np.flatnonzero(~over & (count < 2)).tolist():
        bad = _empty_record(out[v])
        if bad:
            return "node %d: %s" % (v, bad)
    for v in case["nodes"].tolist():
        r = np.array(ranks[v], dtype=np.int64)
        i, j = np.tril_indices(len(r), -1)
        k = r[i] * (r[i] - 1) // 2 + r[j]      # the pair (rank r[j], rank r[i]) in the triangle over every link
        bad = _bars(_Record(out[v]), x[k], y[k], shift_rule=_no_shift_rule)
        if bad:
            return "node %d (%d links): %s" % (v, len(r), bad)
    return None


# ---- hommola ----


def _hommola_draw(rng, L):
    import hommola_clade_reference as ref
    sizes = {s: dict(L, leaves=L["universe"], leaves_lo=3) for s in "xy"}
    if L["big"] and rng.integers(16) == 0:      # the large sort class: a universe above 2048 on one side
        sizes["xy"[int(rng.integers(2))]]["leaves_exact"] = int(rng.integers(2049, 2301))
    case = _two_trees(rng, L, "hommola", sizes=sizes)      # x: the other tree, y: the clade tree
    pc, po = case["parent_y"], case["parent_x"]
    n_links = int(rng.integers(0, 3)) if rng.integers(10) == 0 else int(round(2.0 ** rng.uniform(1.0, math.log2(L["links"] / 2))))
    leaves_c, leaves_o = _leaves_of(pc), _leaves_of(po)
    pool = rng.choice(leaves_c, max(1, int(len(leaves_c) * rng.uniform(0.1, 1.0))), replace=False)
    case["m"] = n_links
    case["ids_y"], case["ids_x"] = rng.choice(pool, n_links).astype(np.int64), rng.choice(leaves_o, n_links).astype(np.int64)
    case["perms"] = int(rng.integers(0, 7))
    case["seed"] = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    lay = ref.Layout(pc, po, case["ids_y"], case["ids_x"])
    nodes = rng.choice(len(pc), min(len(pc), int(rng.integers(1, 9))), replace=False).tolist()
    if rng.integers(2):
        nodes.append(int(np.flatnonzero(pc < 0)[0]))
    if n_links and rng.integers(2):      # a clade above a linked leaf: nested with the root, and with links of its own
        v = int(case["ids_y"][0])
        for _ in range(int(rng.integers(1, 4))):
            v = int(pc[v]) if pc[v] >= 0 else v
        nodes.append(v)
    case["nodes"] = np.array(sorted(set(nodes), key=lambda v: (lay.leaf_begin[v], -lay.leaf_count[v], v)), dtype=np.int64)
    case["chunks"] = [int(v) for v in rng.permutation([0, 1, 2, 3, 1000])[:2]]
    case["_layout"] = lay
    return case


def _sort_class(n):
    return "wave" if n <= 64 else "small" if n <= 2048 else "large"


def _hommola_census(case, C):
    _shared_census(case, C)
    lay, nodes, rows = case["_layout"], case["nodes"].tolist(), case["perms"] + 1
    links = [lay.links(v)[1] for v in nodes]
    C["p = 0 alone"] += case["perms"] == 0
    C["a clade with fewer than two links"] += any(n < 2 for n in links)
    C["nested clades in one call"] += any(lay.leaf_begin[a] <= lay.leaf_begin[b] and lay.leaf_begin[b] + lay.leaf_count[b] <= lay.leaf_begin[a] + lay.leaf_count[a]
                                          for a in nodes for b in nodes if a != b)
    C["disjoint clades in one call"] += any(lay.leaf_begin[a] + lay.leaf_count[a] <= lay.leaf_begin[b] for a in nodes for b in nodes)
    if case["perms"] and any(n >= 2 for n in links):
        C["sort class %s" % _sort_class(len(lay.univ_o))] += 1
        for v, n in zip(nodes, links):
            C["sort class %s" % _sort_class(int(lay.leaf_count[v]))] += n >= 2
    C["other universe larger than clade universe"] += len(lay.univ_o) > len(lay.univ_c)
    C["clade universe larger than other universe"] += len(lay.univ_c) > len(lay.univ_o)
    blocks = np.cumsum([0] + [rows * -(-(n * (n - 1) // 2) // TILE) for n in links])      # a row is cut into blocks of a tile
    for c in case["chunks"]:
        if c > 0:
            C["a chunk that ends inside a clade's rows"] += any(b0 < k * c < b1 for b0, b1 in zip(blocks[:-1], blocks[1:])
                                                                 for k in range(b0 // c, b1 // c + 1))
    C["a row of several blocks"] += any(n * (n - 1) // 2 > TILE for n in links)


def _hommola_check(case, rng, L):
    import hommola_clade_reference as ref
    lay, nodes, perms, seed = case["_layout"], case["nodes"], case["perms"], case["seed"]
    if L["device"] < 0:      # the permutation of the reference against the library's host form
        for v in nodes.tolist():
            for p in {0, perms}:
                for side, n in ((0, int(lay.leaf_count[v])), (1, len(lay.univ_o))):
                    if n >= 1 and not np.array_equal(ref.permutation(seed, v, p, side, n), _capi.hommola_permutation(seed, v, p, side, n, device=-1)):
                        return "sigma of node %d, p %d, side %d over %d positions differs from st_hommola_permutation" % (v, p, side, n)
        return None
    dO, dC = _handles(case)
    clades = np.zeros(len(nodes), dtype=_capi.HOMMOLA_CLADE)
    for i, v in enumerate(nodes.tolist()):
        lo, n = lay.links(v)
        clades[i] = (v, lay.leaf_begin[v], lay.leaf_count[v], lo, n, 0)
    got = dO.hommola_clades_host(dC, lay.univ_o, lay.univ_c, lay.pos_o, lay.pos_c, clades, perms, seed, case["chunks"][0])
    other = dO.hommola_clades_host(dC, lay.univ_o, lay.univ_c, lay.pos_o, lay.pos_c, clades, perms, seed, case["chunks"][1])
    bad = _first_diff(other, got, "chunk_blocks %d against %d, (clade, p)" % (case["chunks"][1], case["chunks"][0]))
    if bad:
        return bad
    for i, v in enumerate(nodes.tolist()):
        ids_o, ids_c = lay.rows(v, perms, seed)
        bad = _first_diff(got[i], dO.compare_rows_host(dC, ids_o, ids_c), "clade %d (node %d, %d links) against st_compare_rows_host, p" % (i, v, ids_o.shape[1]))
        if bad:
            return bad
    return None


# ---- linked: the index mapping of SuchLinkedTrees that needs no GPU ----


def _binary_tree(rng, leaves):
    """an in-order strictly binary tree (what the facade's left / right arrays describe)"""
    kind = int(rng.integers(4))
    if kind == 0:
        return synth.balanced_tree(int(min(7, max(1, round(math.log2(leaves))))), seed=int(rng.integers(1 << 31)))
    if kind == 1:
        return synth.caterpillar_tree(leaves, seed=int(rng.integers(1 << 31)))
    return synth.skewed_tree(rng, leaves, float(rng.choice(SKEWS)))


def _linked_draw(rng, L):
    case = {"family": "linked", "env": {}}
    for s in "ab":
        parent, dist = _binary_tree(rng, int(round(2.0 ** rng.uniform(3.0, math.log2(min(200, 4 * L["universe"] // 2))))))
        case["parent_" + s], case["dist_" + s] = np.asarray(parent, dtype=np.int32), np.asarray(dist, dtype=np.float32)
    na, nb = ((len(case["parent_" + s]) + 1) // 2 for s in "ab")
    mat = (rng.random((na, nb)) < rng.uniform(0.02, 0.5)).astype(np.int64)
    mat[rng.random(na) < 0.2, :] = 0      # empty rows and columns
    mat[:, rng.random(nb) < 0.2] = 0
    case["matrix"] = mat
    case["row_order"] = rng.permutation(na)      # the DataFrame's rows need not follow TreeA's leaf order
    u = int(rng.integers(4))      # no subset, one on A, one on B, both
    case["subset_a"] = int(rng.integers(0, len(case["parent_a"]))) if u in (1, 3) else None
    case["subset_b"] = int(rng.integers(0, len(case["parent_b"]))) if u in (2, 3) else None
    case["of"] = "AB"[int(rng.integers(2))]
    case["tree"] = "AB"[int(rng.integers(2))]      # (the device layer: whose clades linked_distances_by_clade takes)
    case["rows"] = int(rng.integers(1 << 31))
    # hommola_by_clade on the device layer: the other side's subset holds three leaves and more (the call refuses fewer)
    o = "subset_a" if case["tree"] == "B" else "subset_b"
    po = case["parent_a" if case["tree"] == "B" else "parent_b"]
    while case[o] is not None and len(_bfs_leaves(po, case[o])) < 3:
        case[o] = int(po[case[o]])
    n_clade = (len(case["parent_b" if case["tree"] == "B" else "parent_a"]) + 1) // 2
    case["max_leaves"] = int((3, int(rng.integers(3, n_clade + 1)), int(rng.integers(3, max(4, n_clade // 4) + 1)), n_clade)[int(rng.integers(4))])
    case["hperms"], case["hseed"] = int(rng.integers(0, 7)), int(rng.integers(0, 1 << 64, dtype=np.uint64))
    case["group_rows"] = (None, 1, 8, 50)[int(rng.integers(4))]      # _HOMMOLA_GROUP_ROWS forced small
    case["hchunk"] = int((0, 1, 2)[int(rng.integers(3))])
    case["min_partners"] = int(rng.integers(0, 4))
    case["max_partners"] = None if rng.integers(2) else int(rng.integers(1, 8))
    return case


def _bfs_leaves(parent, node):
    """the leaves below a node, breadth-first, the child of the lower id first (in-order ids: the left child)"""
    kids = [[] for _ in range(len(parent))]
    for v in range(len(parent)):
        if parent[v] >= 0:
            kids[parent[v]].append(v)
    out, queue = [], [int(node)]
    for v in queue:
        if kids[v]:
            queue.extend(kids[v])
        else:
            out.append(v)
    return out


def _linked_restated(case):
    """(TreeA subset leaves, TreeB subset leaves, the link list [(b, a)]) from the dense matrix: columns in the order of
    TreeB's subset leaves, within a column the DataFrame's row order, kept where the TreeA leaf is in its subset"""
    pa, pb, mat = case["parent_a"], case["parent_b"], case["matrix"]
    leaves_a = _bfs_leaves(pa, case["subset_a"]) if case["subset_a"] is not None else list(range(0, len(pa), 2))
    leaves_b = _bfs_leaves(pb, case["subset_b"]) if case["subset_b"] is not None else list(range(0, len(pb), 2))
    in_a = set(leaves_a)
    links = [(b, 2 * int(r)) for b in leaves_b for r in case["row_order"] if mat[r, b // 2] and 2 * int(r) in in_a]
    return leaves_a, leaves_b, links


def _linked_census(case, C):
    leaves_a, leaves_b, links = _linked_restated(case)
    case["_restated"] = (leaves_a, leaves_b, links)
    C["of=" + case["of"]] += 1
    C["a subset on A alone"] += case["subset_a"] is not None and case["subset_b"] is None
    C["a subset on B alone"] += case["subset_b"] is not None and case["subset_a"] is None
    C["subsets on both"] += case["subset_a"] is not None and case["subset_b"] is not None
    C["no subset"] += case["subset_a"] is None and case["subset_b"] is None
    C["a subset that is one leaf"] += len(leaves_a) == 1 or len(leaves_b) == 1
    C["no link inside the subsets"] += not links
    linked = {a for _, a in links} if case["of"] == "A" else {b for b, _ in links}
    C["a leaf without links inside the subset"] += len(linked) < len(leaves_a if case["of"] == "A" else leaves_b)
    C["a subset that drops links of a kept leaf"] += any(
        case["matrix"][a // 2].sum() > sum(1 for _, x in links if x == a) for a in {a for _, a in links})
    C["a partner cap"] += case["max_partners"] is not None
    t = case["tree"]
    C["tree=" + t] += 1
    clade, other = (case["subset_a"], case["subset_b"]) if t == "A" else (case["subset_b"], case["subset_a"])
    C["a subset on the clade side alone"] += clade is not None and other is None
    C["a subset on the other side alone"] += other is not None and clade is None
    H = _hommola_rows_restated(case)
    case["_hommola"] = H
    C["hommola_by_clade: rows"] += bool(H["rows"])
    C["a clade in skipped_nodes"] += bool(H["skipped"])
    C["two groups of maximal clades"] += H["groups"] >= 2
    C["_HOMMOLA_GROUP_ROWS forced small"] += case["group_rows"] is not None
    C["a leaf without links inside a clade"] += H["unlinked"]
    C["hommola_by_clade: p = 0 alone"] += case["hperms"] == 0


def _hommola_rows_restated(case):
    """What hommola_by_clade(tree=t, max_leaves=) must report, from the dense matrix and the parent arrays: the links in the
    rank order of the clade tree's root (columns in TreeB's leaf order -- from its root for tree="B", of its subset for
    tree="A" --, the DataFrame's row order within a column, TreeA's subset kept for tree="B"); per inner node of the clade
    tree, breadth-first, its leaves and links; rows with three and more of each, those above max_leaves skipped; and the
    number of library calls: whole maximal clades (within max_leaves, the parent not) in leaf order, a call closed when
    the next clade's rows would pass _HOMMOLA_GROUP_ROWS // (permutations + 1)."""
    t, mat = case["tree"], case["matrix"]
    pa, pb = case["parent_a"], case["parent_b"]
    leaves_a, leaves_b, _ = _linked_restated(case)
    if t == "B":
        in_a = set(leaves_a)
        links = [(b, 2 * int(r)) for b in _bfs_leaves(pb, int(np.flatnonzero(pb < 0)[0])) for r in case["row_order"]
                 if mat[r, b // 2] and 2 * int(r) in in_a]
        pc, clade_of = pb, [b for b, _ in links]
    else:
        links = [(b, 2 * int(r)) for b in leaves_b for r in case["row_order"] if mat[r, b // 2]]
        pc, clade_of = pa, [a for _, a in links]
    n = len(pc)
    kids = [[] for _ in range(n)]
    for v in range(n):
        if pc[v] >= 0:
            kids[pc[v]].append(v)
    n_leaves, n_links, first = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.arange(n)
    for leaf in clade_of:
        n_links[leaf] += 1
    unlinked = np.array([not kids[v] and n_links[v] == 0 for v in range(n)], dtype=np.int64)
    order, queue = [], [int(np.flatnonzero(pc < 0)[0])]
    for v in queue:
        queue.extend(kids[v])
        order.append(v)
    for v in reversed(order):      # children before parents
        if kids[v]:
            n_leaves[v] = sum(n_leaves[c] for c in kids[v])
            n_links[v] = sum(n_links[c] for c in kids[v])
            unlinked[v] = sum(unlinked[c] for c in kids[v])
            first[v] = min(first[c] for c in kids[v])      # (in-order ids: the leaf order is the id order)
        else:
            n_leaves[v] = 1
    kept = [v for v in order if kids[v] and n_leaves[v] >= 3 and n_links[v] >= 3]
    ml = case["max_leaves"]
    rows, skipped = [v for v in kept if n_leaves[v] <= ml], [v for v in kept if n_leaves[v] > ml]
    per_owner = {}
    for v in rows:      # a row's maximal clade: its highest ancestor within max_leaves
        w = v
        while pc[w] >= 0 and n_leaves[pc[w]] <= ml:
            w = int(pc[w])
        per_owner[w] = per_owner.get(w, 0) + 1
    per_group = max(1, (case["group_rows"] or 1 << 21) // (case["hperms"] + 1))
    groups, held = 0, None
    for w in sorted(per_owner, key=lambda u: first[u]):
        if held is None or held + per_owner[w] > per_group:
            groups, held = groups + 1, 0
        held += per_owner[w]
    return {"links": links, "rows": rows, "skipped": skipped, "n_leaves": n_leaves, "n_links": n_links, "groups": groups,
            "unlinked": bool(any(unlinked[v] for v in rows))}


def _linked_state(S):
    return (S.subset_a_root, S.subset_b_root, S.subset_a_size, S.subset_b_size, S.subset_n_links, np.array(S.subset_a_leafs).tobytes(),
            np.array(S.subset_b_leafs).tobytes(), np.array(S.linklist).tobytes(), S._seed)


def _linked_check(case, rng, L):
    import pandas as pd
    from suchtree_amd import SuchTree
    from suchtree_amd.linked import SuchLinkedTrees
    pa, pb, mat = case["parent_a"], case["parent_b"], case["matrix"]
    A = SuchTree((pa, case["dist_a"], ["a%d" % i for i in range(mat.shape[0])]))
    B = SuchTree((pb, case["dist_b"], ["b%d" % i for i in range(mat.shape[1])]))
    name_a, name_b = {v: k for k, v in A.leaves.items()}, {v: k for k, v in B.leaves.items()}
    order = case["row_order"]
    df = pd.DataFrame(mat[order], index=[name_a[2 * int(r)] for r in order], columns=[name_b[2 * c] for c in range(mat.shape[1])])
    S = SuchLinkedTrees(A, B, df)
    if case["subset_a"] is not None:
        S.subset_a(case["subset_a"])
    if case["subset_b"] is not None:
        S.subset_b(case["subset_b"])
    leaves_a, leaves_b, links = case["_restated"]
    if list(S.subset_a_leafs) != leaves_a or list(S.subset_b_leafs) != leaves_b:
        return "the subset's leaves differ from the breadth-first walk of the parent arrays"
    if [tuple(int(v) for v in row) for row in S.linklist] != links:
        return "linklist differs from the dense matrix: got %s want %s" % (S.linklist.tolist()[:6], links[:6])
    before = _linked_state(S)
    a, b = S._links_in_order(S.subset_columns, S.subset_a_leafs)
    if a.tolist() != [x for _, x in links] or b.tolist() != [x for x, _ in links]:
        return "_links_in_order differs from the link list of the same subsets"
    of, lo, hi = case["of"], case["min_partners"], case["max_partners"]
    own, partner, root, rows, sets = S._partner_rows(of, lo, hi)
    want_rows, want_sets = [], []
    for leaf in (leaves_a if of == "A" else leaves_b):
        partners = [b_ if of == "A" else a_ for b_, a_ in links if (a_ if of == "A" else b_) == leaf]
        if len(partners) >= max(lo, 1) and (hi is None or len(partners) <= hi):
            want_rows.append(leaf)
            want_sets.append(partners)
    if (own, partner) != ((A, B) if of == "A" else (B, A)) or root != (S.subset_b_root if of == "A" else S.subset_a_root):
        return "_partner_rows(%s): the wrong trees or partner root" % of
    if [int(v) for v in rows] != want_rows or [np.asarray(s_).tolist() for s_ in sets] != want_sets:
        return "_partner_rows(%s, %s, %s) differs from the dense matrix: rows %s want %s" % (of, lo, hi, list(rows)[:8], want_rows[:8])
    if _linked_state(S) != before:
        return "the subset state, linklist or sampler state changed under _links_in_order / _partner_rows"
    return _linked_device(case, S, A, B, df) if L["device"] >= 0 else None


def _clade_row(R, C, i, node, t, census):
    """test_gpu_clades._check_row as it stands; only where it fails, the same checks with the bars on var, cov and r derived
    for a difference that cancels.  _check_row asks 1e-10 relative of var and cov, and 1e-10 relative (or 1e-12) of the sums
    sxx, syy, sxy about the record's shift, a clade's first pair.  cov = (sxy - sx sy / n) / n and var = (sxx - sx^2 / n) / n:
    a record whose sums meet their own bars may be off by 3e-10 sqrt(sxx syy) / n in cov and by 3e-10 sxx / n in var
    (|sx| <= sqrt(n sxx)).  Where the two columns of a clade happen to be uncorrelated -- linked seed 2 case 3: six pairs, cov
    6.6e-9 beside variances of 6.1 and 0.014 -- or a column is nearly constant, cov or var is orders of magnitude below
    these raw moments, which the float64 reference shows in its own sums, and no record in float64 meets 1e-10 of the
    difference itself (the record there is off by 3.3e-9 of cov, 2e-17 absolute).  There var and cov are held to these
    bounds, r to dcov / sqrt(vx vy) + |r| (dvx / 2 vx + dvy / 2 vy), and p to its own function at the r reported.
    Counted in the census; pinned on constructed columns in tests/test_fuzz_compare_host.py."""
    from scipy.stats import beta
    from test_gpu_clades import _check_row
    try:
        _check_row(R, C, i, node, t)
        return None
    except AssertionError as e:
        first = e
    res = R.linked_distances()      # (R stands at subset_x(node): _check_row put it there)
    x, y = res["TreeA"], res["TreeB"]
    c, n = C.comparison(node), len(x)
    if not (C.n_links[i] == R.subset_n_links and C.n_pairs[i] == n and c.n_pairs == n):
        return "node %d: _check_row: %s" % (node, first)
    r = C.pearson_r[i]
    bad = _derived_moments(c, r, x, y)
    if bad:
        return "node %d: _check_row: %s; and %s" % (node, first, bad)
    if not np.isnan(r):
        at_r = 2 * beta(n / 2 - 1, n / 2 - 1, loc=-1, scale=2).sf(abs(r))
        if not abs(C.pvalue[i] - at_r) <= 1e-9 * at_r + 1e-300:
            return "node %d: pvalue %r, pearsonr's own function at this r %r" % (node, C.pvalue[i], at_r)
    census["clade row: var, cov and r held to the bound derived from the raw moments about the shift"] += 1
    return None


def _derived_moments(c, r, x, y):
    """The bars of _check_moments on a record c (and its r) over the columns x, y with var, cov and r held to the bounds
    derived in _clade_row's docstring, 3e-10 of the raw moments about the record's shift; a message, or None.
    tests/test_fuzz_compare_host.py pins it on a constructed column."""
    n = len(x)
    dx, dy = x - c.shift_x, y - c.shift_y
    sxx, syy, sxy = (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()
    near = lambda g, w: _rel(g, w) < 1e-10 or abs(g - w) < 1e-12      # noqa: E731
    plain = (_rel(c.mean_x, x.mean()) < 1e-10 and _rel(c.mean_y, y.mean()) < 1e-10 and near(c.sxx, sxx) and near(c.syy, syy)
             and near(c.sxy, sxy) and abs(c.sx - dx.sum()) <= 1e-10 * np.sqrt(n * c.sxx) and abs(c.sy - dy.sum()) <= 1e-10 * np.sqrt(n * c.syy)
             and (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max()))
    if not plain:
        return "a mean, a sum about the shift, a minimum or a maximum outside the bars of _check_moments"
    vx, vy, cov = np.var(x), np.var(y), np.cov(x, y, bias=True)[0, 1]
    dvx, dvy, dcov = 3e-10 * sxx / n, 3e-10 * syy / n, 3e-10 * np.sqrt(sxx * syy) / n
    if not (abs(c.var_x - vx) <= dvx and abs(c.var_y - vy) <= dvy and abs(c.cov - cov) <= dcov):
        return "var or cov outside the bounds derived from the raw moments about the shift"
    if min(vx, c.var_x) <= dvx or min(vy, c.var_y) <= dvy:      # a variance within its bound of zero: r is NaN or anything
        return None
    want = cov / np.sqrt(vx * vy)
    if not abs(r - want) <= dcov / np.sqrt(vx * vy) + abs(want) * (dvx / (2 * vx) + dvy / (2 * vy)) + 1e-12:
        return "pearson_r %r against %r, outside the derived bound" % (r, want)
    return None


def _linked_device(case, S, A, B, df):
    """linked_distances_by_clade(tree=t) row by row against a second object that loops subset_x(c) and reduces
    linked_distances() in float64 (the bars of test_gpu_clades._check_row, through _clade_row, on twelve drawn rows of a
    case); the rows are the internal nodes, breadth-first, with two links and more under the other side's current subset;
    the state is the same bytes afterwards; then hommola_by_clade (_linked_hommola)"""
    from suchtree_amd.linked import SuchLinkedTrees
    t = case["tree"]
    before = _linked_state(S)
    C = S.linked_distances_by_clade(tree=t)
    if _linked_state(S) != before:
        return "the subset state, linklist or sampler state changed under linked_distances_by_clade(tree=%s)" % t
    R = SuchLinkedTrees(A, B, df)
    other = case["subset_a"] if t == "B" else case["subset_b"]
    if other is not None:
        (R.subset_a if t == "B" else R.subset_b)(other)
    clade = B if t == "B" else A
    want = []
    for v in clade.get_internal_nodes():
        (R.subset_b if t == "B" else R.subset_a)(int(v))
        if R.subset_n_links >= 2:
            want.append(int(v))
    if C.nodes.tolist() != want:
        return "linked_distances_by_clade(tree=%s): rows %s, the per-clade loop keeps %s" % (t, C.nodes.tolist()[:10], want[:10])
    pick = np.random.default_rng(case["rows"]).permutation(len(want))[:12]
    for i in sorted(pick.tolist()):
        bad = _clade_row(R, C, i, want[i], t, case["_census"])
        if bad:
            return bad
    return _linked_hommola(case, S, R, A, B)


def _linked_hommola(case, S, R, A, B):
    """hommola_by_clade(tree=t, keep_stats=True, max_leaves=drawn) against the per-clade loop of the second object R (which
    holds the other side's subset): the rows and skipped_nodes are the loop's, the link and leaf counts subset_x(c)'s, the
    observed r hommola_cospeciation(0)'s within 1e-12 (both NaN where a column is constant), as
    test_fixtures_against_the_per_clade_loop asks; every permuted r equals, byte for byte, the r of st_compare_rows_host on
    the rows of hommola_clade_reference.Layout over the restated links; n_ge, n_nan and p_value follow from these.  That
    comparison of the permuted r is a consistency check between two library paths (st_hommola_clades_host behind the facade
    against st_compare_rows_host and compare.row_stats on ids restated here): what is independent in it is the relabelling,
    the layout and the grouping, not the float arithmetic, which the rows and hommola families hold.  The number of
    st_hommola_clades_host calls is counted through a wrapper and must be the restated grouping's, so that "two groups of
    maximal clades" in the census is what the library did.  The
    counts and the arithmetic of p are held on every row, r and the permuted rows on twelve drawn rows of a case."""
    import hommola_clade_reference as ref
    from suchtree_amd.compare import _SUMS, row_stats
    from suchtree_amd.linked import SuchLinkedTrees
    t, perms, seed, ml, want = case["tree"], case["hperms"], case["hseed"], case["max_leaves"], case["_hommola"]
    before = _linked_state(S)
    default, entry, calls = SuchLinkedTrees._HOMMOLA_GROUP_ROWS, _capi.DeviceTree.hommola_clades_host, []

    def counted(self, *args, **kw):      # the library calls of this hommola_by_clade: one per group of maximal clades
        calls.append(len(args[5]))
        return entry(self, *args, **kw)
    try:
        _capi.DeviceTree.hommola_clades_host = counted
        if case["group_rows"] is not None:
            SuchLinkedTrees._HOMMOLA_GROUP_ROWS = case["group_rows"]
        H = S.hommola_by_clade(tree=t, permutations=perms, seed=seed, keep_stats=True, max_leaves=ml, chunk_blocks=case["hchunk"])
    finally:
        SuchLinkedTrees._HOMMOLA_GROUP_ROWS, _capi.DeviceTree.hommola_clades_host = default, entry
    if len(calls) != want["groups"] or sum(calls) != len(want["rows"]):
        return "hommola_by_clade made %d calls of st_hommola_clades_host over %s clades; the grouping restated for the census gives %d over %d" % (
            len(calls), calls[:8], want["groups"], len(want["rows"]))
    if _linked_state(S) != before:
        return "the subset state, linklist or sampler state changed under hommola_by_clade(tree=%s)" % t
    clade, other = (B, A) if t == "B" else (A, B)
    subset_clade = R.subset_b if t == "B" else R.subset_a
    rows, skipped, links_of, leaves_of = [], [], {}, {}
    for v in clade.get_internal_nodes():
        subset_clade(int(v))
        size = R.subset_b_size if t == "B" else R.subset_a_size
        if R.subset_n_links >= 3 and size >= 3:
            (rows if size <= ml else skipped).append(int(v))
            links_of[int(v)], leaves_of[int(v)] = R.subset_n_links, size
    if rows != want["rows"] or skipped != want["skipped"]:
        return "the per-clade loop's rows %s / skipped %s differ from the restatement's %s / %s" % (
            rows[:8], skipped[:8], want["rows"][:8], want["skipped"][:8])
    if H.nodes.tolist() != rows or H.skipped_nodes.tolist() != skipped:
        return "hommola_by_clade(tree=%s, max_leaves=%d): rows %s skipped %s, the per-clade loop gives %s and %s" % (
            t, ml, H.nodes.tolist()[:8], H.skipped_nodes.tolist()[:8], rows[:8], skipped[:8])
    if H.n_links.tolist() != [links_of[v] for v in rows] or H.n_leaves.tolist() != [leaves_of[v] for v in rows]:
        return "hommola_by_clade: n_links or n_leaves differ from subset_x(c)'s"
    if (H.permutations, H.seed, H.tree) != (perms, seed, t) or (len(rows) and H.perm_stats.shape != (len(rows), perms)):
        return "hommola_by_clade: permutations, seed, tree or the shape of perm_stats"
    ids_clade = np.array([b if t == "B" else a for b, a in want["links"]], dtype=np.int64)
    ids_other = np.array([a if t == "B" else b for b, a in want["links"]], dtype=np.int64)
    other_root = case["subset_a"] if t == "B" else case["subset_b"]
    lay = ref.Layout(clade._flat.parent, other._flat.parent, ids_clade, ids_other, other_root) if rows else None
    dev_o, dev_c = other._device_tree(), clade._device_tree()
    pick = set(np.random.default_rng(case["rows"] + 1).permutation(len(rows))[:12].tolist())
    for i, v in enumerate(rows):
        stats, r = H.perm_stats[i], H.corr_coeff[i]
        with np.errstate(invalid="ignore"):
            if H.n_ge[i] != np.count_nonzero(stats >= r) or H.n_nan[i] != np.count_nonzero(np.isnan(stats)):
                return "node %d: n_ge or n_nan do not follow from perm_stats" % v
        if not ((math.isnan(r) and math.isnan(H.p_value[i])) or H.p_value[i] == (H.n_ge[i] + 1) / (perms + 1)):
            return "node %d: p_value %r with n_ge %d of %d permutations" % (v, H.p_value[i], H.n_ge[i], perms)
        if i not in pick:
            continue
        subset_clade(v)
        loop = R.hommola_cospeciation(0).corr_coeff
        if not ((math.isnan(loop) and math.isnan(r)) or abs(r - loop) < 1e-12):
            return "node %d: corr_coeff %r, the per-clade loop's %r" % (v, r, loop)
        ids_o, ids_c = lay.rows(v, perms, seed)
        m = dev_o.compare_rows_host(dev_c, ids_o, ids_c)
        bad = _first_diff(stats, row_stats(m["n"], *(m[k] for k in _SUMS))[5][1:], "node %d: perm_stats against the reference rows, p - 1" % v)
        if bad:
            return bad
    return None


def _with_census(fn):
    """the checker sees the session's census, to count what only it can know: a canopy handle the shape refused, a merge
    held to its derived bound"""
    def census(case, C):
        case["_census"] = C
        fn(case, C)
    return census


DRAW = {"moments": _moments_draw, "ranks": lambda r, L: _stat_draw(r, L, "ranks"), "kendall2": lambda r, L: _stat_draw(r, L, "kendall2"),
        "rows": _rows_draw, "quartets": _quartets_draw, "clades": _clades_draw, "hommola": _hommola_draw, "linked": _linked_draw}
CENSUS = {"moments": _with_census(_moments_census), "ranks": _with_census(_stat_census), "kendall2": _with_census(_stat_census),
          "rows": _with_census(_rows_census),
          "quartets": _with_census(_quartets_census), "clades": _with_census(_clades_census),
          "hommola": _with_census(_hommola_census), "linked": _with_census(_linked_census)}
CHECK = {"moments": _moments_check, "ranks": lambda c, r, L: _stat_check(c, r, L, "ranks"),
         "kendall2": lambda c, r, L: _stat_check(c, r, L, "kendall2"), "rows": _rows_check, "quartets": _quartets_check,
         "clades": _clades_check, "hommola": _hommola_check, "linked": _linked_check}

# What a session must have reached at least once.  The host layer's sizes stop at 64 leaves and 40 ids: the chunk, tile and
# window edges are the device layer's alone.  "-0.0 and +0.0 in one column" is counted and not required: a sum of branch
# lengths that starts at +0.0 never gives -0.0 (tests/test_gpu_rank_edges.py says the same), so no tree delivers it.
_HOST_SHARED = _SHARED
_LINKED = ["of=A", "of=B", "a subset on A alone", "a subset on B alone", "subsets on both", "no subset", "a subset that is one leaf",
                        "no link inside the subsets", "a leaf without links inside the subset", "a subset that drops links of a kept leaf",
                        "a partner cap"]
REQUIRED = {
    "host": {"moments": _HOST_SHARED + ["n = 0", "n = 1", "n = 2", "entry triangle", "entry pairs", "range begins in mid-row", "edges in LDS",
                                        "edges in global memory", "values outside the edges", "a constant column (r is NaN)", "no histogram"],
             "ranks": _HOST_SHARED + ["n = 0", "n = 1", "entry triangle", "entry pairs", "an infinity", "a tie group of all pairs",
                                      "one occupied bucket", "several buckets", "negative and positive values in one column", "a zero distance"],
             "kendall2": _HOST_SHARED + ["n = 0", "n = 1", "entry triangle", "entry pairs", "an infinity", "a tie group of all pairs", "repeated pairs"],
             "rows": _HOST_SHARED + ["m below 2", "rows of at most 64 pairs (lane form)", "rows just above 64 pairs (m = 12)", "one row"],
             "quartets": _HOST_SHARED + ["class 3 present", "every class of distinct leaves present", "a polytomy side", "m = 4", "entry all",
                                         "entry sample", "entry explicit", "a range that begins past 0", "several chunks", "an empty range",
                                         "tree_x is tree_y"],
             "clades": _HOST_SHARED + ["a piece of at most 64 pairs", "a piece above 64 pairs", "a triangle segment (several links on one leaf)",
                                       "a node over the cap", "no cap", "no links", "a caterpillar clade tree", "a polytomy in the clade tree",
                                       "a leaf without links inside a clade with links"],
             "hommola": _HOST_SHARED + ["p = 0 alone", "a clade with fewer than two links", "nested clades in one call", "disjoint clades in one call",
                                        "sort class wave", "sort class small", "other universe larger than clade universe",
                                        "clade universe larger than other universe"],
             "linked": _LINKED},
    "device": {"moments": _SHARED + ["n = 0", "n = 1", "n = 2", "entry triangle", "entry pairs", "range begins in mid-row", "fewer than 4096 pairs",
                                     "more than 4096 pairs", "edges in LDS", "edges in global memory", "values outside the edges",
                                     "a constant column (r is NaN)", "a second chunk of pairs", "no histogram", "tree_x is tree_y"],
               "ranks": _SHARED + ["n = 0", "n = 1", "entry triangle", "entry pairs", "two chunks", "a sub-range that splits a chunk",
                                   "one occupied bucket", "several buckets", "an infinity", "a tie group of all pairs",
                                   "negative and positive values in one column", "a zero distance"],
               "kendall2": _SHARED + ["n = 0", "n = 1", "entry triangle", "entry pairs", "one tile less one", "one tile", "one tile and one",
                                      "a tie group wider than a tile", "two chunks", "repeated pairs", "an infinity"],
               "rows": _SHARED + ["m below 2", "rows of at most 64 pairs (lane form)", "rows just above 64 pairs (m = 12)", "dense layout",
                                  "padded layout", "a short last block summed by lane 0", "several blocks a row", "more rows than a chunk holds",
                                  "one row"],
               "quartets": _SHARED + ["class 3 present", "every class of distinct leaves present", "a polytomy side", "m = 4", "entry all",
                                         "entry sample", "entry explicit", "a range that begins past 0", "several chunks", "an empty range",
                                         "tree_x is tree_y"],
               "clades": _SHARED + ["a piece of at most 64 pairs", "a piece above 64 pairs", "a triangle segment (several links on one leaf)",
                                       "a node over the cap", "no cap", "no links", "a caterpillar clade tree", "a polytomy in the clade tree",
                                       "a leaf without links inside a clade with links"] + ["a segment cut by a tile boundary", "two chunks", "tree_x is tree_y"],
               "linked": _LINKED + ["tree=A", "tree=B", "a subset on the clade side alone", "a subset on the other side alone", "hommola_by_clade: rows",
                                    "a clade in skipped_nodes", "two groups of maximal clades", "_HOMMOLA_GROUP_ROWS forced small",
                                    "a leaf without links inside a clade", "hommola_by_clade: p = 0 alone"],
               "hommola": _SHARED + ["p = 0 alone", "a clade with fewer than two links", "nested clades in one call", "disjoint clades in one call",
                                        "sort class wave", "sort class small", "other universe larger than clade universe",
                                        "clade universe larger than other universe"] + ["sort class large", "a chunk that ends inside a clade's rows", "a row of several blocks"]},
}


def census(family, seed, cases, layer):
    return fuzz_analyses.census(family, seed, cases, layer, tables=sys.modules[__name__])


def missing(family, C, layer):
    return fuzz_analyses.missing(family, C, layer, tables=sys.modules[__name__])


def run(family, seed, cases, layer, first=0, require=True):
    """one session under fuzz_analyses.run's rules (the compare families set no environment variables)"""
    return fuzz_analyses.run(family, seed, cases, layer, lambda k, v: None, first, require, tables=sys.modules[__name__])


if __name__ == "__main__":
    family = sys.argv[1]
    n_cases, seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000, int(sys.argv[3]) if len(sys.argv) > 3 else 1
    layer0 = sys.argv[4] if len(sys.argv) > 4 else "host"
    got = run(family, seed0, n_cases, layer0, first=int(sys.argv[5]) if len(sys.argv) > 5 else 0, require=False)
    print("fuzz %s: %d cases, seed %d, layer %s, no mismatch; reached:" % (family, n_cases, seed0, layer0))
    for key in sorted(got):
        print("  %-55s %d" % (key, got[key]))
    print("  never reached: %s" % missing(family, got, layer0))
