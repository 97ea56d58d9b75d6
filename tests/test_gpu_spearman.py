"""Exact Spearman rank correlation on the GPU (compare_distances(spearman=True), linked_distances_summary(spearman=True),
C ABI st_compare_*_ranks_host): the 128-bit integer rank sums against st_spearman_host on the oracle's float32
distances -- equal, not close -- and spearman_r against scipy."""
import ctypes
import dataclasses
import os

import numpy as np
import pandas as pd
import pytest
from scipy.stats import spearmanr

from conftest import golden_path
from oracle.oracle import OracleTree
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu
CORES = len(os.sched_getaffinity(0))
RANK_FIELDS = ("spearman_r", "rank_sxy", "rank_sxx", "rank_syy", "distinct_x", "distinct_y")


def _tri_pairs(ids):
    rows, cols = np.tril_indices(len(ids), -1)
    return np.stack([ids[cols], ids[rows]], axis=1).astype(np.int64)


def _f32(d):
    f = d.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), d, equal_nan=True)      # the oracle's distances are float32 sums
    return f


def _same_sums(got, want):
    for k, _ in _capi.RankSums._fields_:
        assert getattr(got, k) == getattr(want, k), (k, getattr(got, k), getattr(want, k))


def _same_as_host(c, x, y):
    """The rank fields of DistanceComparison c against st_spearman_host and scipy on the float32 columns x, y."""
    want = _capi.spearman_host(x, y)
    assert (c.rank_sxy, c.rank_sxx, c.rank_syy) == (want.sxy, want.sxx, want.syy)
    assert (c.distinct_x, c.distinct_y) == (want.distinct_x, want.distinct_y) == (len(np.unique(x)), len(np.unique(y)))
    rs = spearmanr(x, y)[0]
    print("spearman_r %.17g, scipy %.17g, difference %.3g" % (c.spearman_r, rs, c.spearman_r - rs))
    assert abs(c.spearman_r - rs) < 1e-12
    return want


@pytest.fixture(scope="module")
def ml_nj(ml_arrays, nj_arrays):
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    return SuchTree((p1, d1)), SuchTree((p2, d2)), OracleTree(p1, d1), OracleTree(p2, d2), leaves1, nj_of


@pytest.fixture(scope="module")
def sample600(ml_nj):
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    sel = np.random.default_rng(22).choice(len(leaves1), 600, replace=False)
    ids_x, ids_y = leaves1[sel], nj_of[sel]
    return ids_x, ids_y, _f32(O1.distances_mt(_tri_pairs(ids_x), CORES)), _f32(O2.distances_mt(_tri_pairs(ids_y), CORES))


def test_exact_on_3000_shared_leaves_of_ml_and_nj(ml_nj):
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    sel = np.random.default_rng(21).choice(len(leaves1), 3000, replace=False)
    ids_x, ids_y = leaves1[sel], nj_of[sel]
    x, y = _f32(O1.distances_mt(_tri_pairs(ids_x), CORES)), _f32(O2.distances_mt(_tri_pairs(ids_y), CORES))
    assert len(x) == 4_498_500
    c = T1.compare_distances(T2, leaves=(ids_x, ids_y), spearman=True)
    _same_as_host(c, x, y)
    assert abs(c.spearman_r - 0.96160767801838) < 1e-12
    plain = T1.compare_distances(T2, leaves=(ids_x, ids_y))
    for f in dataclasses.fields(c):
        if f.name in RANK_FIELDS:
            assert getattr(plain, f.name) is None
        else:      # every other field: the same bits
            a, b = getattr(c, f.name), getattr(plain, f.name)
            assert a is b is None or a == b or (np.isnan(a) and np.isnan(b)), f.name
    # with a histogram: the histogram calls as they are without ranks, the ranks beside them
    h = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=16, spearman=True)
    h0 = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=16)
    assert np.array_equal(h.hist, h0.hist) and (h.sx, h.sxx, h.sxy, h.pearson_r) == (h0.sx, h0.sxx, h0.sxy, h0.pearson_r)
    assert (h.rank_sxy, h.rank_sxx, h.rank_syy, h.spearman_r) == (c.rank_sxy, c.rank_sxx, c.rank_syy, c.spearman_r)


def test_chunks_and_repeats_return_the_same_bytes(ml_nj, sample600):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample600
    dx, dy = T1._device_tree(), T2._device_tree()
    assert len(x) == 179_700                      # 21 chunks of 8192 and a tail, 2 of 65536 and a tail
    want = _capi.spearman_host(x, y)
    m0, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    seen = []
    for chunk in (8192, 65536, 0, 0):
        m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, chunk_pairs=chunk)
        _same_sums(r, want)
        assert bytes(m) == bytes(m0)              # the moments of the existing call, whatever the chunk
        seen.append(bytes(r))
    assert len(set(seen)) == 1
    for bad in (-8192, 100, 8191):
        with pytest.raises(ValueError):
            dx.compare_triangle_ranks_host(dy, ids_x, ids_y, chunk_pairs=bad)


def test_sub_ranges_agree_with_the_host_on_the_slice(ml_nj, sample600):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample600
    dx, dy = T1._device_tree(), T2._device_tree()
    K = len(x)
    for k0, kc, chunk in ((0, K // 3, 0), (K // 3, K - K // 3, 16384), (12345, 8192 + 3, 8192), (K - 1, 1, 0), (7, 2, 0)):
        m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, k0, kc, chunk_pairs=chunk)
        _same_sums(r, _capi.spearman_host(x[k0:k0 + kc], y[k0:k0 + kc]))
        assert bytes(m) == bytes(dx.compare_triangle_host(dy, ids_x, ids_y, k0, kc)[0])
    m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, 5, 0)
    assert m.n == 0 and (r.n, r.n_nan, r.sxy, r.sxx, r.syy, r.distinct_x) == (0, 0, 0, 0, 0, 0)


def test_explicit_pairs_with_self_pairs_ancestors_and_internal_nodes(ml_nj):
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    rng = np.random.default_rng(5)
    px = rng.integers(0, T1.size, (40_000, 2))               # any node, internal ones included
    py = rng.integers(0, T2.size, (40_000, 2))
    px[:500, 1] = px[:500, 0]                                # (a, a)
    py[250:750, 1] = py[250:750, 0]
    par1, par2 = T1._flat.parent.astype(np.int64), T2._flat.parent.astype(np.int64)
    up = px[1000:1400, 0].copy()
    for _ in range(3):                                       # a node and an ancestor of it, in both orders
        up = np.where(par1[up] >= 0, par1[up], up)
    px[1000:1400, 1] = up
    px[1400:1800] = px[1000:1400, ::-1]
    up = py[1000:1400, 0].copy()
    for _ in range(2):
        up = np.where(par2[up] >= 0, par2[up], up)
    py[1200:1600, 1] = up[:400]
    py[1200:1600, 0] = py[1000:1400, 0]
    x, y = _f32(O1.distances_mt(px, CORES)), _f32(O2.distances_mt(py, CORES))
    assert (x == 0).sum() >= 500 and (y == 0).sum() >= 500
    c = T1.compare_distances(T2, pairs=(px, py), spearman=True)
    want = _same_as_host(c, x, y)
    dx, dy = T1._device_tree(), T2._device_tree()
    for chunk in (8192, 0):
        _same_sums(dx.compare_pairs_ranks_host(dy, px, py, chunk_pairs=chunk)[1], want)


def test_synthetic_trees_negative_zero_lengths_and_massive_ties():
    # negative and zero branch lengths
    p, d = synth.random_binary_tree(1500, seed=9)
    rng = np.random.default_rng(10)
    d2 = np.asarray(d, dtype=np.float64).copy()
    d2[rng.random(len(d2)) < 0.3] = 0.0
    neg = rng.random(len(d2)) < 0.2
    d2[neg] = -np.abs(d2[neg]) - 0.01
    root = int(np.flatnonzero(np.asarray(p) < 0)[0])
    d2[root] = 0.0
    d2 = d2.astype(np.float32)
    A, B = SuchTree((p, d)), SuchTree((p, d2))
    OA, OB = OracleTree(np.asarray(p), np.asarray(d)), OracleTree(np.asarray(p), d2)
    ids = np.arange(0, 2 * 1500 - 1, 2, dtype=np.int64)      # in-order ids: the leaves are the even ones
    x, y = _f32(OA.distances_mt(_tri_pairs(ids), CORES)), _f32(OB.distances_mt(_tri_pairs(ids), CORES))
    assert (y < 0).any() and (y == 0).any()
    _same_as_host(A.compare_distances(B, leaves=(ids, ids), spearman=True), x, y)
    # a caterpillar with one branch length: a few thousand distinct values among 2 million pairs
    pc, dc = synth.caterpillar_tree(2000)
    dc = np.where(np.asarray(pc) < 0, 0.0, 0.25).astype(np.asarray(dc).dtype)
    C = SuchTree((pc, dc))
    OC = OracleTree(np.asarray(pc), dc)
    idc = np.arange(0, 2 * 2000 - 1, 2, dtype=np.int64)
    perm = np.random.default_rng(11).permutation(2000)
    xc, yc = _f32(OC.distances_mt(_tri_pairs(idc), CORES)), _f32(OC.distances_mt(_tri_pairs(idc[perm]), CORES))
    c = C.compare_distances(C, leaves=(idc, idc[perm]), spearman=True)
    _same_as_host(c, xc, yc)
    assert c.distinct_x < 5000 and c.n_pairs == 1_999_000
    # the same tree and the same ids twice: Sxy == Sxx == Syy and r == 1.0 exactly
    s = C.compare_distances(C, leaves=(idc, idc), spearman=True)
    assert s.rank_sxy == s.rank_sxx == s.rank_syy > 0 and s.spearman_r == 1.0


def test_walk_strategy_feeds_the_same_ranks(ml_nj, sample600):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample600
    A, B = SuchTree((T1._flat.parent, T1._flat.distance)), SuchTree((T2._flat.parent, T2._flat.distance))
    A._device_tree().set_strategy("walk")
    B._device_tree().set_strategy("walk")
    _same_as_host(A.compare_distances(B, leaves=(ids_x, ids_y), spearman=True), x, y)


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
def test_linked_distances_summary_spearman(which):
    SLT = _slt(which)
    res = SLT.linked_distances()
    s = SLT.linked_distances_summary(spearman=True)
    assert s.n_pairs == res["n_pairs"]
    _same_as_host(s, _f32(np.asarray(res["TreeA"])), _f32(np.asarray(res["TreeB"])))
    plain = SLT.linked_distances_summary()
    assert plain.spearman_r is None and (plain.sx, plain.sxx, plain.sxy, plain.pearson_r) == (s.sx, s.sxx, s.sxy, s.pearson_r)
    sb = SLT.linked_distances_summary(bins=8, spearman=True)
    assert sb.hist.sum() == s.n_pairs and (sb.rank_sxy, sb.spearman_r) == (s.rank_sxy, s.spearman_r)


def test_more_than_2_31_pairs_is_refused_at_once(ml_nj):
    T1, T2, _, _, leaves1, nj_of = ml_nj
    ids_x, ids_y = np.resize(leaves1, 70_000), np.resize(nj_of, 70_000)
    assert 70_000 * 69_999 // 2 > 2**31 - 1
    out, ranks, bad = _capi.PairMoments(), _capi.RankSums(), ctypes.c_int64(0)
    dx, dy = T1._device_tree(), T2._device_tree()
    rc = _capi.load().st_compare_triangle_ranks_host(dx.handle, dy.handle, ids_x.ctypes.data, ids_y.ctypes.data, 70_000, 0,
                                                     70_000 * 69_999 // 2, 0, ctypes.byref(out), ctypes.byref(ranks), ctypes.byref(bad))
    assert rc == _capi.ST_ERR_ARG and "2^31 - 1" in _capi.last_error()
    with pytest.raises(ValueError):
        T1.compare_distances(T2, leaves=(ids_x, ids_y), spearman=True)
    # a range of it that fits is served
    m, r = dx.compare_triangle_ranks_host(dy, ids_x, ids_y, 2**31, 20_000)
    assert r.n == 20_000 and m.n == 20_000
