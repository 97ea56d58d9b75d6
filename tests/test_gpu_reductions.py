"""The GPU reductions of the compare paths at their edges: k_pair_shift / k_pair_moments (st_compare_triangle_host,
st_compare_pairs_host) across chunk boundaries and in every histogram layout, k_row_blocks (st_compare_rows_host) and
k_clade_pieces (st_compare_clades_host) at their lane / wave thresholds, every kernel family under the same reductions,
and non-finite distances.  Each group checks the GPU against float64 sums on the host over the per-pair distances of
triangle_host / distances_host / the oracle (pinned bit for bit to each other by test_gpu_parity.py), and asserts that
it reached the case it is named for by restating the library's rule."""
import ctypes

import numpy as np
import pytest
from scipy.stats import beta, pearsonr

from compare_reference import SHIFT_PAIRS, _Sums, _check_shift, _rel
from conftest import golden_path
from oracle.oracle import OracleTree
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.compare import DistanceComparison, histogram_edges
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu

TILE = _capi.CLADE_TILE              # ST_CLADE_TILE
CHUNK_TRIANGLE = 1 << 25             # host_compare.h: kCompareChunkTriangle
CHUNK_PAIRS = 1 << 22                # host_compare.h: kCompareChunkPairs
CHUNK_CLADES = 1 << 25               # compare_plan.h: kCladeChunkPairs (also the rows' default chunk)
ROWS_CHUNK_BLOCKS = 1 << 18          # compare_plan.h: kRowsChunkBlocks
MAX_CELLS = 16384                    # kernels_compare.h: kCmpMaxCells
LANE_PIECE = 64                      # kernels_clades.h: kCladeLanePiece
PROBE_MIN_PAIRS = 1 << 22            # launch_policy.h: kProbeMinPairs
FIELDS = _capi.PAIR_MOMENTS.names


def _check_moments(c, x, y):      # (the bars of tests/test_gpu_compare.py)
    assert c.n_pairs == len(x)
    for got, want in ((c.mean_x, x.mean()), (c.mean_y, y.mean()), (c.var_x, np.var(x)), (c.var_y, np.var(y)),
                      (c.cov, np.cov(x, y, bias=True)[0, 1])):
        assert _rel(got, want) < 1e-10 or abs(got - want) < 1e-12, (got, want)
    dx, dy = x - c.shift_x, y - c.shift_y
    for got, want in ((c.sxx, (dx * dx).sum()), (c.syy, (dy * dy).sum()), (c.sxy, (dx * dy).sum())):
        assert _rel(got, want) < 1e-10 or abs(got - want) < 1e-12, (got, want)
    assert abs(c.sx - dx.sum()) <= 1e-10 * np.sqrt(len(x) * c.sxx) and abs(c.sy - dy.sum()) <= 1e-10 * np.sqrt(len(y) * c.syy)
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max())
    if np.var(x) > 0 and np.var(y) > 0:
        assert abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-12
    else:
        assert np.isnan(c.pearson_r)


def _record(rec):
    """A st_pair_moments record (numpy row) as a DistanceComparison."""
    return DistanceComparison.from_sums(*(rec[k] for k in FIELDS))


@pytest.fixture(scope="module")
def ml_nj(ml_arrays, nj_arrays):
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    return _capi.DeviceTree(p1, d1), _capi.DeviceTree(p2, d2), leaves1, nj_of


# ---- A. moments across chunk boundaries --------------------------------------------------------------------------

def test_triangle_moments_across_the_chunk_boundary(ml_nj):
    dx, dy, leaves1, nj_of = ml_nj
    sel = np.random.default_rng(81).choice(len(leaves1), 8193, replace=False)
    ids_x, ids_y = leaves1[sel], nj_of[sel]
    K = 8193 * 8192 // 2
    assert K == CHUNK_TRIANGLE + 4096
    # (a first pass for the edges: the 64 x 48 histogram spans the data with a clipped top row)
    m_all, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    edges = (np.linspace(m_all.min_x, m_all.max_x, 65), np.linspace(m_all.min_y, (m_all.min_y + m_all.max_y) / 2, 49))
    ranges = [(0, K, True), (5, CHUNK_TRIANGLE + 3, True), (0, CHUNK_TRIANGLE, False)] + [(0, c, False) for c in (1, 3, 4095, 4097)]
    for b, c, _ in ranges:
        # compare_run: chunks of kCompareChunkTriangle counted from k_begin; the ranges sit at the boundary or inside one chunk
        chunks = -(-c // CHUNK_TRIANGLE)
        assert chunks == (2 if c > CHUNK_TRIANGLE else 1)
    assert (CHUNK_TRIANGLE + 3) % CHUNK_TRIANGLE == 3      # (the second chunk of (5, 2^25 + 3) is a 3-pair tail alone)
    got, sums = [], []
    for b, c, with_hist in ranges:
        m, _ = dx.compare_triangle_host(dy, ids_x, ids_y, b, c)
        mh, h = dx.compare_triangle_host(dy, ids_x, ids_y, b, c, edges=edges) if with_hist else (None, None)
        if mh is not None:
            assert bytes(mh) == bytes(m)      # (the histogram does not change the sums)
        got.append((m, h))
        sums.append(_Sums(m.shift_x, m.shift_y, edges if with_hist else None))
    block = 1 << 22
    for k0 in range(0, K, block):
        k1 = min(K, k0 + block)
        x, _ = dx.triangle_host(ids_x, k0, k1 - k0)
        y, _ = dy.triangle_host(ids_y, k0, k1 - k0)
        for (b, c, _), (m, _), s in zip(ranges, got, sums):
            lo, hi = max(b, k0), min(b + c, k1)
            if lo < hi:
                s.add(x[lo - k0:hi - k0], y[lo - k0:hi - k0])
            if k0 <= b < k1:
                _check_shift(m, x[b - k0:b - k0 + c], y[b - k0:b - k0 + c])      # (the first 4096 pairs of every range lie in one block)
    for (b, c, _), (m, h), s in zip(ranges, got, sums):
        s.check(m, h)
        r = DistanceComparison.from_moments(m).pearson_r
        assert np.isnan(r) if c == 1 else np.isfinite(r), (c, r)
    assert got[0][1].sum() < K and got[0][1].sum() == sums[0].hist.sum()      # (the range clips)
    # merge: two calls split at a point that is not a chunk multiple equal the single call
    cut = (1 << 24) + 12345
    lo = dx.compare_triangle_host(dy, ids_x, ids_y, 0, cut, edges=edges)
    hi = dx.compare_triangle_host(dy, ids_x, ids_y, cut, K - cut, edges=edges)
    full = DistanceComparison.from_moments(got[0][0], got[0][1], *edges)
    merged = DistanceComparison.merge(DistanceComparison.from_moments(*lo, *edges), DistanceComparison.from_moments(*hi, *edges))
    assert merged.n_pairs == K and np.array_equal(merged.hist, full.hist)
    assert (merged.min_x, merged.max_x, merged.min_y, merged.max_y) == (full.min_x, full.max_x, full.min_y, full.max_y)
    for k in ("mean_x", "mean_y", "var_x", "var_y", "cov", "pearson_r"):
        assert _rel(getattr(merged, k), getattr(full, k)) < 1e-12, k


def test_explicit_pairs_across_chunk_boundaries(ml_nj):
    dx, dy, leaves1, nj_of = ml_nj
    n = 2 * CHUNK_PAIRS + 3
    idx = np.random.default_rng(82).integers(0, len(leaves1), (n, 2))
    px, py = leaves1[idx], nj_of[idx]
    x, _ = dx.distances_host(px)
    y, _ = dy.distances_host(py)
    edges = (np.linspace(x.min(), np.quantile(x, 0.9), 41), np.linspace(y.min(), y.max(), 51))
    for count, with_hist in ((n, True), (CHUNK_PAIRS, False), (CHUNK_PAIRS + 1, True)):
        assert -(-count // CHUNK_PAIRS) == {n: 3, CHUNK_PAIRS: 1, CHUNK_PAIRS + 1: 2}[count]      # chunks of st_compare_pairs_host
        m, h = dx.compare_pairs_host(dy, px[:count], py[:count], edges=edges if with_hist else None)
        _check_shift(m, x, y)
        s = _Sums(m.shift_x, m.shift_y, edges if with_hist else None)
        for k0 in range(0, count, 1 << 22):
            s.add(x[k0:min(count, k0 + (1 << 22))], y[k0:min(count, k0 + (1 << 22))])
        s.check(m, h)


# ---- B. histogram layouts ----------------------------------------------------------------------------------------

def _hist_layout(bins_x, bins_y):
    """MomentsReduce::start (host_compare.h): uint32 counters ((cells + 1) & ~1) * 4 bytes, the edges beside them in LDS
    iff counters + edges <= 128 KiB (else k_pair_moments reads them from global memory), hipFuncSetAttribute iff the
    dynamic LDS exceeds 64 KiB - 1024.  Returns (edges_in_lds, attribute)."""
    cells = bins_x * bins_y
    lds = ((cells + 1) & ~1) * 4
    edges = (bins_x + bins_y + 2) * 8
    in_lds = lds + edges <= 128 * 1024
    if in_lds:
        lds += edges
    return in_lds, lds > 64 * 1024 - 1024


@pytest.fixture(scope="module")
def sample3000(ml_nj):
    dx, dy, leaves1, nj_of = ml_nj
    sel = np.random.default_rng(21).choice(len(leaves1), 3000, replace=False)
    ids_x, ids_y = leaves1[sel], nj_of[sel]
    x, _ = dx.triangle_host(ids_x)
    y, _ = dy.triangle_host(ids_y)
    return ids_x, ids_y, x, y


def test_histogram_layouts(ml_nj, sample3000):
    dx, dy = ml_nj[:2]
    ids_x, ids_y, x, y = sample3000
    m0, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    _check_moments(DistanceComparison.from_moments(m0), x, y)
    full = [(x.min(), x.max()), (y.min(), y.max())]
    shapes = {(128, 128): (True, True), (127, 129): (True, True), (2, 8192): (False, True), (1, 16384): (False, True),
              (16384, 1): (False, True), (1, 16000): (False, False), (7, 9): (True, False)}
    cases = [(s, histogram_edges(s, full, None)) for s in shapes]
    rng = np.random.default_rng(5)
    # edges drawn from the float32 data themselves: many values fall exactly on an edge, the last edge is the maximum
    on_x = np.unique(np.concatenate([rng.choice(x, 40), [x.max()]]))
    on_y = np.unique(np.concatenate([rng.choice(y, 25), [y.max()]]))
    cases.append((None, (on_x, on_y)))
    # repeated edges, a zero-width bin inside and a zero-width last bin
    qx, qy = np.quantile(x, [0.0, 0.2, 0.5, 0.8, 1.0]), np.quantile(y, [0.0, 0.3, 0.6, 1.0])
    rep_x = np.array([qx[0], qx[1], qx[1], qx[2], qx[3], qx[4], qx[4]])
    rep_y = np.array([qy[0], qy[1], qy[2], qy[2], qy[3], qy[3]])
    cases.append((None, (rep_x, rep_y)))
    cases.append((None, histogram_edges((33, 17), [(np.quantile(x, 0.1), np.quantile(x, 0.7)), (np.quantile(y, 0.2), np.quantile(y, 0.95))], None)))
    seen = set()
    for shape, edges in cases:
        bx, by = len(edges[0]) - 1, len(edges[1]) - 1
        layout = _hist_layout(bx, by)
        if shape is not None:
            assert layout == shapes[shape], (shape, layout)
        seen.add(layout)
        m, h = dx.compare_triangle_host(dy, ids_x, ids_y, edges=edges)
        assert bytes(m) == bytes(m0), (bx, by)
        want = np.histogram2d(x, y, bins=edges)[0].astype(np.int64)
        assert np.array_equal(h, want), (bx, by, int(np.abs(h - want).sum()))
    assert seen == {(True, True), (False, True), (False, False), (True, False)}, seen
    assert np.count_nonzero(np.isin(x, on_x)) >= len(on_x) and np.count_nonzero(y == on_y[-1]) > 0
    # 16,385 cells: refused before anything is launched -- by the binding, and by the library itself
    with pytest.raises(ValueError):
        dx.compare_triangle_host(dy, ids_x, ids_y, edges=(np.linspace(0, 1, 2), np.linspace(0, 1, MAX_CELLS + 2)))
    ex, ey = np.linspace(0, 1, 6), np.linspace(0, 1, 3278)
    assert 5 * 3277 == MAX_CELLS + 1
    hist = np.full(5 * 3277, -7, dtype=np.int64)
    out, bad = _capi.PairMoments(), ctypes.c_int64(0)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = dx._lib.st_compare_triangle_host(dx.handle, dy.handle, ptr(ids_x), ptr(ids_y), len(ids_x), 0, len(x), ptr(ex), 5,
                                          ptr(ey), 3277, ctypes.byref(out), ptr(hist), ctypes.byref(bad))
    assert rc == _capi.ST_ERR_ARG and np.all(hist == -7) and out.n == 0


def test_histogram_through_compare_distances(ml_arrays, nj_arrays, sample3000):
    ids_x, ids_y, x, y = sample3000
    T1, T2 = SuchTree((ml_arrays[0], ml_arrays[1])), SuchTree((nj_arrays[0], nj_arrays[1]))
    for bins in (128, (127, 129), (1, 16000)):
        c = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=bins)
        want, wx, wy = np.histogram2d(x, y, bins)
        assert np.array_equal(c.xedges, wx) and np.array_equal(c.yedges, wy)
        assert np.array_equal(c.hist, want.astype(np.int64)) and c.hist.sum() == len(x)
    with pytest.raises(ValueError):
        T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=(5, 3277))


# ---- C. row blocks at their thresholds ---------------------------------------------------------------------------

def _rows_layout(n_rows, m, chunk_pairs):
    """compare_plan.cpp: rows_layout -- (P, S, nb, chunk, dense)."""
    C = chunk_pairs if chunk_pairs > 0 else CHUNK_CLADES
    P = m * (m - 1) // 2
    nb = -(-P // TILE)
    if P <= C // 2:
        max_rows = max(1, min(n_rows, C // P, ROWS_CHUNK_BLOCKS // nb))
        return P, P, nb, max_rows * P, True
    return P, nb * TILE, nb, C, False


def _row_paths(P, nb):
    """kernels_rows.h: k_row_blocks -- one lane per row (P <= kCladeLanePiece), else a wave per block and lane 0 for a
    last block of at most kCladeLanePiece pairs."""
    if P <= LANE_PIECE:
        return {"lane_row"}
    last = P - (nb - 1) * TILE
    return {"wave"} | ({"short_last"} if last <= LANE_PIECE else {"wave_last"})


@pytest.fixture(scope="module")
def trees():
    pa, da = synth.random_binary_tree(3000, seed=7)
    pb, db = synth.random_binary_tree(2000, seed=8)
    return _capi.DeviceTree(pa, da), _capi.DeviceTree(pb, db), pa, pb


def _leaves(parent):
    return np.flatnonzero(np.bincount(parent[parent >= 0], minlength=len(parent)) == 0).astype(np.int64)


def test_row_blocks_at_their_thresholds(trees):
    dA, dB, pa, pb = trees
    la, lb = _leaves(pa), _leaves(pb)
    paths, layouts = set(), set()
    for m in (2, 11, 12, 128, 129, 130):
        rng = np.random.default_rng(1000 + m)
        X, Y = rng.choice(la, (40, m)), rng.choice(lb, (40, m))
        X57, Y57 = X.copy(), Y.copy()
        X57[[0, 29]], Y57[[0, 29]] = X[[29, 0]], Y[[29, 0]]
        want = None
        for chunk in (0, TILE):
            P, S, nb, C, dense = _rows_layout(len(X), m, chunk)
            assert dense == (chunk == 0 or P <= TILE // 2), (m, chunk)
            layouts.add(dense)
            paths |= _row_paths(P, nb)
            out = dA.compare_rows_host(dB, X, Y, chunk)
            swapped = dA.compare_rows_host(dB, X57, Y57, chunk)
            alone = dA.compare_rows_host(dB, X[29:30], Y[29:30], chunk)
            want = out.tobytes() if want is None else want
            assert out.tobytes() == want, (m, chunk)
            assert swapped[0:1].tobytes() == out[29:30].tobytes() == alone.tobytes() and swapped[29:30].tobytes() == out[0:1].tobytes()
        for i in (0, 1, 29, 39):
            x, _ = dA.triangle_host(X[i])
            y, _ = dB.triangle_host(Y[i])
            assert out[i]["shift_x"] == x[0] and out[i]["shift_y"] == y[0]      # (a block's shift: its first pair)
            _check_moments(_record(out[i]), x, y)
    assert paths == {"lane_row", "wave", "short_last", "wave_last"}, paths
    assert layouts == {True, False}, layouts


def test_many_tiny_rows_span_three_chunks(trees):
    dA, dB, pa, pb = trees
    la, lb = _leaves(pa), _leaves(pb)
    n_rows = 2 * ROWS_CHUNK_BLOCKS + 1001
    P, S, nb, C, dense = _rows_layout(n_rows, 3, 0)
    assert dense and -(-n_rows * S // C) == 3      # three chunks: the first piece buffer is used twice
    rng = np.random.default_rng(3)
    X, Y = rng.choice(la, (n_rows, 3)), rng.choice(lb, (n_rows, 3))
    out = dA.compare_rows_host(dB, X, Y)
    # pair k of a row: (ids[j], ids[i]), k = i(i-1)/2 + j
    cols = [(0, 1), (0, 2), (1, 2)]
    x = np.stack([dA.distances_host(np.ascontiguousarray(X[:, [j, i]]))[0] for j, i in cols], 1)
    y = np.stack([dB.distances_host(np.ascontiguousarray(Y[:, [j, i]]))[0] for j, i in cols], 1)
    assert np.array_equal(out["n"], np.full(n_rows, 3)) and np.array_equal(out["shift_x"], x[:, 0]) and np.array_equal(out["shift_y"], y[:, 0])
    dx, dy = x - x[:, :1], y - y[:, :1]
    for k, want in (("sx", dx.sum(1)), ("sy", dy.sum(1)), ("sxx", (dx * dx).sum(1)), ("syy", (dy * dy).sum(1)), ("sxy", (dx * dy).sum(1)),
                    ("min_x", x.min(1)), ("max_x", x.max(1)), ("min_y", y.min(1)), ("max_y", y.max(1))):
        assert np.all(np.abs(out[k] - want) <= 1e-12 * np.abs(want) + 1e-13), k
    for r in (0, ROWS_CHUNK_BLOCKS - 1, ROWS_CHUNK_BLOCKS, 2 * ROWS_CHUNK_BLOCKS, n_rows - 1):
        assert dA.compare_rows_host(dB, X[r:r + 1], Y[r:r + 1]).tobytes() == out[r:r + 1].tobytes(), r


# ---- D. clade pieces at their thresholds -------------------------------------------------------------------------

def _pieces(segs):
    """The pieces of a clade plan as st_compare_clades_host cuts them (compare_plan.cpp: clade_tables and
    clade_fold): segment s's part of each tile it meets -- (tile, lo, hi, s)."""
    out = []
    for s, g in enumerate(segs):
        f, n = int(g["first_pair"]), int(g["n_pairs"])
        for t in range(f // TILE, (f + n - 1) // TILE + 1):
            out.append((t, max(f, t * TILE), min(f + n, (t + 1) * TILE), s))
    return out


def _cherries(parent):
    kids = [[] for _ in parent]
    for v, p in enumerate(parent):
        if p >= 0:
            kids[p].append(v)
    leaf = np.array([not k for k in kids])
    return [tuple(k) for k in kids if len(k) == 2 and leaf[k[0]] and leaf[k[1]]]


def _check_row(S, C, i, node):      # (tests/test_gpu_clades.py::_check_row, tree B)
    S.subset_b(int(node))
    res = S.linked_distances()
    x, y = res["TreeA"], res["TreeB"]
    assert C.n_links[i] == S.subset_n_links and C.n_leaves[i] == S.subset_b_size and C.n_pairs[i] == len(x)
    c = C.comparison(node)
    _check_moments(c, x, y)
    if np.var(x) > 0 and np.var(y) > 0:
        r, p = pearsonr(x, y)
        assert abs(C.pearson_r[i] - r) < 1e-12
        n = len(x)
        at_r = 2 * beta(n / 2 - 1, n / 2 - 1, loc=-1, scale=2).sf(abs(C.pearson_r[i]))
        assert abs(C.pvalue[i] - at_r) <= 1e-9 * at_r + 1e-300, (C.pvalue[i], at_r)


def _clade_system():
    pa, da = synth.balanced_tree(8)
    pb, db = synth.random_binary_tree(600, seed=12)
    A = SuchTree((pa, da, ["a%d" % i for i in range(256)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(600)]))
    leaf_col = {int(v): i for i, v in enumerate(B.leaf_node_ids)}
    rng = np.random.default_rng(12)
    mat = np.zeros((256, 600), dtype=np.int64)
    mat[rng.integers(0, 256, 600), np.arange(600)] = 1      # one link per leaf: cherries give 1-pair rectangles
    ch = _cherries(pb)
    # 8 x 8 = 64 pairs and 5 x 13 = 65 pairs (rectangles of two cherries), 130 x 130 = 16,900 pairs (at least three tiles)
    for (u, v), (ku, kv) in zip(ch[-3:], ((8, 8), (5, 13), (130, 130))):
        for leaf, k in ((u, ku), (v, kv)):
            mat[:, leaf_col[leaf]] = 0
            mat[rng.choice(256, k, replace=False), leaf_col[leaf]] = 1
    import pandas as pd
    return A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves))


def _plan_of(S, B):
    # the links as linked_distances_by_clade(tree="B") hands them to the library (rank order)
    col_of = np.full(B.size, -1, dtype=np.int64)
    col_of[S._col_ids.astype(np.int64)] = np.arange(len(S._col_ids))
    _, ids_b = S._links_in_order(col_of[S._leaf_order(B, B.root_node)], S._subset_a_leafs)
    plan = _capi.clade_plan(B._flat.parent, ids_b)
    return plan, plan["segments"]


def _assert_piece_cases(segs):
    pieces = _pieces(segs)
    lens = np.array([hi - lo for _, lo, hi, _ in pieces])
    per_tile = np.bincount([t for t, _, _, _ in pieces])
    seg_tiles = np.array([(int(g["first_pair"]) + int(g["n_pairs"]) - 1) // TILE - int(g["first_pair"]) // TILE + 1 for g in segs])
    first = np.array([int(segs[s]["first_pair"]) for _, _, _, s in pieces])
    end = first + np.array([int(segs[s]["n_pairs"]) for _, _, _, s in pieces])
    lo, hi = np.array([p[1] for p in pieces]), np.array([p[2] for p in pieces])
    assert np.count_nonzero(segs["n_pairs"] == 1) > 64                    # 1-pair segments
    assert per_tile.max() > LANE_PIECE                                    # a tile of more than one round of 64 pieces
    assert np.any(lens == LANE_PIECE) and np.any(lens == LANE_PIECE + 1)  # the last lane piece and the first wave piece
    assert seg_tiles.max() >= 3                                           # a segment over at least three tiles
    assert np.any((lo > first) & (hi < end))                              # a piece cut by a tile boundary on both sides
    assert np.any((lo > first) & (hi == end)) and np.any((lo == first) & (hi < end))
    assert np.all(lens > 0) and lens.sum() == int(segs["n_pairs"].sum())


def test_clade_pieces_at_their_thresholds():
    A, B, df = _clade_system()
    S = SuchLinkedTrees(A, B, df)
    _, segs = _plan_of(S, B)
    _assert_piece_cases(segs)
    C = S.linked_distances_by_clade()
    assert len(C) >= 590
    R = SuchLinkedTrees(A, B, df)
    for i, node in enumerate(C.nodes):
        _check_row(R, C, i, node)
    for chunk in (TILE, 3 * TILE):
        K = S.linked_distances_by_clade(chunk_pairs=chunk)
        for col in ("n_pairs", "shift_x", "shift_y", "sx", "sy", "sxx", "syy", "sxy", "min_a", "max_a", "min_b", "max_b"):
            assert getattr(K, col).tobytes() == getattr(C, col).tobytes(), (chunk, col)


# ---- E. every kernel family produces the same reductions ---------------------------------------------------------

def _skewed_candidates():
    rng = np.random.default_rng(404)      # (test_gpu_parity.py::test_lineage_sum_mode_of_the_deep_kernel's small deep trees)
    for n, skew in ((30000, 0.97), (9000, 0.995), (11000, 0.9), (16000, 0.9)):
        yield synth.skewed_tree(rng, n, skew)


class _Calls:
    """The four reductions over one fixed input, tree X = a configured handle, tree Y = the other tree's defaults."""

    def __init__(self, dy, parent_y, ids_x, ids_y, px, py, seed):
        self.dy, self.parent_y, self.ids_x, self.ids_y, self.px, self.py = dy, parent_y, ids_x, ids_y, px, py
        rng = np.random.default_rng(seed)
        self.rx = np.stack([ids_x[rng.permutation(len(ids_x))] for _ in range(20)])
        self.ry = np.stack([ids_y[rng.permutation(len(ids_y))] for _ in range(20)])
        self.edges = None

    def run(self, dx):
        if self.edges is None:
            m, _ = dx.compare_triangle_host(self.dy, self.ids_x, self.ids_y)
            self.edges = (np.linspace(m.min_x, m.max_x, 65), np.linspace(m.min_y, m.max_y, 65))
        tri = dx.compare_triangle_host(self.dy, self.ids_x, self.ids_y, edges=self.edges)
        pairs = dx.compare_pairs_host(self.dy, self.px, self.py)
        clades = dx.compare_clades_host(self.dy, self.parent_y, self.ids_x, self.ids_y)
        rows = dx.compare_rows_host(self.dy, self.rx, self.ry)
        return tri, pairs, clades, rows

    @staticmethod
    def key(res):
        (tm, th), (pm, _), (cm, cc), rows = res
        return bytes(tm) + th.tobytes(), bytes(pm), cm.tobytes() + cc.tobytes(), rows.tobytes()

    def check_float64(self, dx, res):
        (tm, th), (pm, _), (cm, _), rows = res
        x, _ = dx.triangle_host(self.ids_x)
        y, _ = self.dy.triangle_host(self.ids_y)
        _check_moments(DistanceComparison.from_moments(tm), x, y)
        assert np.array_equal(th, np.histogram2d(x, y, bins=self.edges)[0].astype(np.int64))
        root = int(np.flatnonzero(self.parent_y < 0)[0])      # (the root clade: every pair of the links, lower rank first)
        _check_moments(_record(cm[root]), x, y)
        px, _ = dx.distances_host(self.px)
        py, _ = self.dy.distances_host(self.py)
        _check_moments(DistanceComparison.from_moments(pm), px, py)
        for i in (0, 19):
            x, _ = dx.triangle_host(self.rx[i])
            y, _ = self.dy.triangle_host(self.ry[i])
            _check_moments(_record(rows[i]), x, y)


def test_every_kernel_family_gives_the_same_reductions(ml_arrays, nj_arrays):
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    rng = np.random.default_rng(91)
    sel = rng.choice(len(leaves1), 3000, replace=False)
    idx = rng.integers(0, len(leaves1), (PROBE_MIN_PAIRS + 17, 2))
    assert len(idx) >= PROBE_MIN_PAIRS      # (the batch probe looks at batches from kProbeMinPairs pairs)
    dml, dnj = _capi.DeviceTree(p1, d1), _capi.DeviceTree(p2, d2)
    seen = set()

    def sweep(calls, default, configs):
        base = calls.run(default)
        calls.check_float64(default, base)
        want = calls.key(base)
        seen.add(default.info()["big_batch_kernel"])
        for name, dev in configs():
            kernel = dev.info()["big_batch_kernel"]
            seen.add(kernel)
            got = calls.key(calls.run(dev))
            for what, g, w in zip(("triangle", "pairs", "clades", "rows"), got, want):
                assert g == w, (name, kernel, what)

    # X = nj.tree, Y = ml.tree's defaults
    def nj_configs():
        dev = _capi.DeviceTree(p2, d2)
        for sort, walk, ladder in ((1, 0, 0), (0, 0, 0), (1, 1, 0), (0, 0, 1)):
            dev.set_option("tile_sort", sort)
            dev.set_option("prefer_walk_sorted", walk)
            dev.set_option("ladder_scalar", ladder)
            yield "nj tile_sort=%d prefer_walk_sorted=%d ladder_scalar=%d" % (sort, walk, ladder), dev
        dev.set_strategy("walk")
        for wl in (0, 1):
            dev.set_option("walk_ladder", wl)
            yield "nj walk walk_ladder=%d" % wl, dev
        dev.close()

    sweep(_Calls(dml, p1, nj_of[sel], leaves1[sel], nj_of[idx], leaves1[idx], 1), dnj, nj_configs)

    # X = ml.tree, Y = nj.tree's defaults
    def ml_configs():
        dev = _capi.DeviceTree(p1, d1)
        for k, v in (("tile_sort", 0), ("ladder_scalar", 1), ("ladder_min_pairs", 0), ("prefer_walk_sorted", 0)):
            dev.set_option(k, v)
        for sums in (0, 1):
            dev.set_option("ladder_sums", sums)
            assert dev.info()["big_batch_kernel"] == "canopy_ladder" and dev.info()["ladder_sums"] == sums
            yield "ml ladder_sums=%d" % sums, dev
        dev.set_strategy("walk")
        for wl in (0, 1):
            dev.set_option("walk_ladder", wl)
            yield "ml walk walk_ladder=%d" % wl, dev
        dev.close()
        for mb, dropped in ((16, "rec_i"), (8, "canopy")):
            dev = _capi.DeviceTree(p1, d1, table_mb=mb)
            assert dropped in dev.info()["dropped_tables"], dev.info()
            yield "ml table_mb=%d" % mb, dev
            dev.close()

    sweep(_Calls(dnj, p2, leaves1[sel], nj_of[sel], leaves1[idx], nj_of[idx], 2), dml, ml_configs)

    # X = a small deep tree whose big-batch kernel can be the tile-sorted canopy kernel, Y = ml.tree's defaults
    for parent, dist in _skewed_candidates():
        dev = _capi.DeviceTree(parent, dist)
        for k, v in (("tile_sort", 1), ("ladder_scalar", 0), ("prefer_walk_sorted", 0)):
            dev.set_option(k, v)
        if dev.info()["big_batch_kernel"] == "canopy_sorted":
            break
        dev.close()
    else:
        pytest.fail("no small deep tree runs the tile-sorted canopy kernel")
    lx = _leaves(parent)
    r2 = np.random.default_rng(93)
    calls = _Calls(dml, p1, r2.choice(lx, 3000, replace=False), leaves1[sel], r2.choice(lx, (PROBE_MIN_PAIRS, 2)), leaves1[idx[:PROBE_MIN_PAIRS]], 3)
    sweep(calls, _capi.DeviceTree(parent, dist), lambda: iter([("deep canopy_sorted", dev)]))
    dev.close()
    assert seen == {"canopy", "canopy_ladder", "canopy_sorted", "walk_sorted", "walk"}, seen


# ---- F. non-finite values ----------------------------------------------------------------------------------------

def _special_tree(nan_leaves):
    """test_gpu_parity.py::test_special_float_values's lengths (denormal, -0.0, 3e38, -1.5, eps, FLT_MIN), and NaN on
    ``nan_leaves`` of the leaves."""
    parent, dist = synth.random_binary_tree(3000, seed=4)
    rng = np.random.default_rng(4)
    dist = dist.copy()
    k = rng.integers(0, len(dist), 600)
    dist[k[:100]] = np.float32(1e-42)
    dist[k[100:200]] = np.float32(-0.0)
    dist[k[200:300]] = np.float32(3e38)
    dist[k[300:400]] = np.float32(-1.5)
    dist[k[400:500]] = np.float32(2.220446e-16)
    dist[k[500:]] = np.float32(1.17549435e-38)
    leaves = _leaves(parent)
    nan = leaves[rng.choice(len(leaves), nan_leaves, replace=False)]
    dist[nan] = np.float32(np.nan)
    return parent, dist, leaves, nan


def _check_nonfinite(rec, x, y, hist=None, edges=None, merged=False):
    """shift finite, min / max NaN-ignoring, each sum within the float64 bar where numpy's is finite and otherwise of
    numpy's class (without float64 overflow that class does not depend on the order).  ``merged``: pieces summed about
    their own shifts and merged on the host (clades, rows); the class of an infinite cross product (x - cx)(y - cy)
    depends on the shift it was summed about, so a non-finite sxy is only required to be non-finite there."""
    assert rec["n"] == len(x)
    assert np.isfinite(rec["shift_x"]) and np.isfinite(rec["shift_y"])
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = x - rec["shift_x"], y - rec["shift_y"]
        want = {"sx": dx.sum(), "sy": dy.sum(), "sxx": (dx * dx).sum(), "syy": (dy * dy).sum(), "sxy": (dx * dy).sum()}
    for k, w in want.items():
        g = rec[k]
        if np.isfinite(w):
            if k in ("sx", "sy"):
                sq = want["s" + k[1] * 2]
                assert abs(g - w) <= 1e-10 * np.sqrt(len(x) * sq), (k, g, w)
            else:
                assert _rel(g, w) < 1e-10 or abs(g - w) < 1e-12, (k, g, w)
        elif merged and k == "sxy":
            assert not np.isfinite(g), (k, g, w)
        elif np.isnan(w):
            assert np.isnan(g), (k, g)
        else:
            assert g == w, (k, g, w)
    for k, v in (("x", x), ("y", y)):
        if np.all(np.isnan(v)):
            assert rec["min_" + k] == np.inf and rec["max_" + k] == -np.inf
        else:
            assert rec["min_" + k] == np.nanmin(v) and rec["max_" + k] == np.nanmax(v), k
    if edges is not None:
        assert np.array_equal(hist, np.histogram2d(x, y, bins=edges)[0].astype(np.int64))


def _as_rec(m):
    return {k: getattr(m, k) for k in FIELDS}


def test_non_finite_values(trees):
    _, dB, _, pb = trees
    parent, dist, leaves, nan = _special_tree(3)
    dX = _capi.DeviceTree(parent, dist)
    OX = OracleTree(parent, dist)
    lb = _leaves(pb)
    rng = np.random.default_rng(6)
    finite_leaves = np.setdiff1d(leaves, nan)
    cand = rng.choice(finite_leaves, (4000, 2))
    cd = OX.distances(cand)
    inf_pairs = cand[np.isinf(cd)]
    assert len(inf_pairs) > 10 and not np.isnan(cd).any()
    assert not np.isfinite(OX.distances(np.array([[nan[0], finite_leaves[0]]], np.int64))).any()
    # compare: an inf pair first (the shift's sample is not finite), then a NaN pair first
    for first in (inf_pairs[0], np.array([nan[0], finite_leaves[0]])):
        ids_x = np.concatenate([first, rng.choice(np.setdiff1d(finite_leaves, first), 1498, replace=False)])
        ids_y = rng.choice(lb, 1500, replace=False)
        x, _ = dX.triangle_host(ids_x)
        y, _ = dB.triangle_host(ids_y)
        assert not np.isfinite(x[:SHIFT_PAIRS].sum())
        m, _ = dX.compare_triangle_host(dB, ids_x, ids_y)
        assert m.shift_x == 0.0
        edges = (np.linspace(np.nanmin(x), np.median(x[np.isfinite(x)]), 33), np.linspace(y.min(), y.max(), 17))
        mh, h = dX.compare_triangle_host(dB, ids_x, ids_y, edges=edges)
        assert bytes(mh) == bytes(m)
        _check_nonfinite(_as_rec(m), x, y, h, edges)
        assert 0 < h.sum() < np.count_nonzero(np.isfinite(x))      # (inf, NaN and the clipped top all left out)
    # rows of 129 ids: row 0's first pair is NaN, row 1's second block starts on an inf pair (pair 8192 = (ids[64], ids[128]))
    n_rows, m = 6, 129
    X = np.stack([rng.choice(np.setdiff1d(finite_leaves, inf_pairs[1]), m, replace=False) for _ in range(n_rows)])
    Y = rng.choice(lb, (n_rows, m))
    X[0, 0] = nan[1]
    X[1, 64], X[1, 128] = inf_pairs[1]
    assert 128 * 127 // 2 + 64 == TILE
    out = dX.compare_rows_host(dB, X, Y)
    for i in range(n_rows):
        x, _ = dX.triangle_host(X[i])
        y, _ = dB.triangle_host(Y[i])
        if i == 0:
            assert np.isnan(x[0]) and out[0]["shift_x"] == 0.0
        if i == 1:
            assert np.isinf(x[TILE])
        _check_nonfinite(out[i], x, y, merged=True)
    # clades: links on the special tree's leaves, some NaN ones; pieces whose first pair is not finite
    pyb = pb
    n_links = 900
    link_x = rng.choice(leaves, n_links)
    link_x[:20] = nan[2]
    link_y = rng.choice(lb, n_links)
    plan = _capi.clade_plan(pyb, link_y)
    perm, segs = plan["perm"], plan["segments"]
    firsts = []
    for g in segs:      # the first pair of a segment: (r0, c0), or (r0, r0 + 1) for a triangle, lower rank first
        p, q = int(g["row_begin"]), int(g["col_begin"]) if g["kind"] == _capi.CLADE_RECT else int(g["row_begin"]) + 1
        a, b = sorted((perm[p], perm[q]))
        firsts.append((link_x[a], link_x[b]))
    fx = OX.distances(np.array(firsts, np.int64))
    assert np.any(np.isnan(fx)) and np.any(np.isinf(fx)) and np.any(np.isfinite(fx))
    res, count = dX.compare_clades_host(dB, pyb, link_x, link_y)
    checked = 0
    for v in np.flatnonzero(count >= 2):
        pos = np.sort(perm[plan["begin"][v]:plan["begin"][v] + count[v]])
        if len(pos) > 400 and checked > 40:
            continue
        i, j = np.tril_indices(len(pos), -1)
        px = np.stack([link_x[pos[j]], link_x[pos[i]]], 1)
        py = np.stack([link_y[pos[j]], link_y[pos[i]]], 1)
        _check_nonfinite(res[v], OX.distances(px), dB.distances_host(py)[0], merged=True)
        checked += 1
    assert checked > 40


def test_compare_distances_range_from_nan_data():
    """compare_distances(bins=int, range=None) takes its range from the NaN-ignoring min / max; numpy raises."""
    pa, da = synth.balanced_tree(6)
    da = da.copy()
    leaves = _leaves(pa)
    da[leaves[5]] = np.float32(np.nan)
    T, U = SuchTree((pa, da)), SuchTree(synth.balanced_tree(6))
    c = T.compare_distances(U, leaves=(leaves, leaves), bins=8)
    x, _ = T._device_tree().triangle_host(leaves)
    y, _ = U._device_tree().triangle_host(leaves)
    assert np.isnan(x).sum() == 63 and np.all(np.isfinite(y))
    assert (c.min_x, c.max_x) == (np.nanmin(x), np.nanmax(x)) and np.isnan(c.mean_x)
    ex, ey = histogram_edges(8, None, (np.nanmin(x), np.nanmax(x), y.min(), y.max()))
    assert np.array_equal(c.xedges, ex) and np.array_equal(c.yedges, ey)
    assert np.array_equal(c.hist, np.histogram2d(x, y, bins=(ex, ey))[0].astype(np.int64)) and c.hist.sum() == len(x) - 63
    with pytest.raises(ValueError):
        np.histogram2d(x, y, 8)
