"""The compare path on the GPU (SuchTree.compare_distances, SuchLinkedTrees.linked_distances_summary, C ABI
st_compare_*): moments and 2-D histograms of two trees' distances over the same pairs, against numpy float64 on the
oracle's distances."""
import ctypes
import json
import os
import time

import numpy as np
import pandas as pd
import pytest
from scipy.stats import pearsonr

from conftest import golden_path
from oracle.oracle import OracleTree
from suchtree_amd import InvalidNodeError, SuchTree, _capi, synth
from suchtree_amd.compare import DistanceComparison
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu
KNOWN = json.load(open(golden_path("known_answers.json")))
CORES = len(os.sched_getaffinity(0))


def _tri_pairs(ids):
    rows, cols = np.tril_indices(len(ids), -1)
    return np.stack([ids[cols], ids[rows]], axis=1).astype(np.int64)


@pytest.fixture(scope="module")
def ml_nj(ml_arrays, nj_arrays):
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    return SuchTree((p1, d1)), SuchTree((p2, d2)), OracleTree(p1, d1), OracleTree(p2, d2), leaves1, nj_of


@pytest.fixture(scope="module")
def sample3000(ml_nj):
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    sel = np.random.default_rng(21).choice(len(leaves1), 3000, replace=False)
    ids_x, ids_y = leaves1[sel], nj_of[sel]
    x = O1.distances_mt(_tri_pairs(ids_x), CORES)
    y = O2.distances_mt(_tri_pairs(ids_y), CORES)
    return ids_x, ids_y, x, y


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_moments(c, x, y):
    assert c.n_pairs == len(x)
    for got, want in ((c.mean_x, x.mean()), (c.mean_y, y.mean()), (c.var_x, np.var(x)), (c.var_y, np.var(y)),
                      (c.cov, np.cov(x, y, bias=True)[0, 1])):
        assert _rel(got, want) < 1e-10, (got, want)
    dx, dy = x - c.shift_x, y - c.shift_y
    for got, want in ((c.sxx, (dx * dx).sum()), (c.syy, (dy * dy).sum()), (c.sxy, (dx * dy).sum())):
        assert _rel(got, want) < 1e-10, (got, want)
    assert abs(c.sx - dx.sum()) < 1e-10 * np.sqrt(len(x) * c.sxx) and abs(c.sy - dy.sum()) < 1e-10 * np.sqrt(len(y) * c.syy)
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max())
    assert abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-12


def test_exact_on_3000_shared_leaves_of_ml_and_nj(ml_nj, sample3000):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample3000
    assert len(x) == 4_498_500
    rng = [(np.quantile(x, 0.03), np.quantile(x, 0.97)), (np.quantile(y, 0.05), np.quantile(y, 0.99))]
    c = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=64, range=rng)
    want, wx, wy = np.histogram2d(x, y, bins=64, range=rng)
    assert c.hist.dtype == np.int64 and c.hist.shape == (64, 64)
    assert np.array_equal(c.hist, want.astype(np.int64)) and np.array_equal(c.xedges, wx) and np.array_equal(c.yedges, wy)
    assert c.hist.sum() < len(x)                      # the range clips
    assert c.n_leaves == 3000
    _check_moments(c, x, y)
    # numpy's default range (two passes)
    c2 = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=64)
    want2, wx2, wy2 = np.histogram2d(x, y, 64)
    assert np.array_equal(c2.hist, want2.astype(np.int64)) and np.array_equal(c2.xedges, wx2) and np.array_equal(c2.yedges, wy2)
    assert c2.hist.sum() == len(x)
    # non-uniform edges, two different bin counts
    ex = np.unique(np.quantile(x, np.linspace(0, 1, 33)))
    ey = np.unique(np.quantile(y, np.linspace(0, 1, 200)))
    c3 = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=(ex, ey))
    assert np.array_equal(c3.hist, np.histogram2d(x, y, bins=(ex, ey))[0].astype(np.int64))
    # moments only: the same sums as with a histogram
    c4 = T1.compare_distances(T2, leaves=(ids_x, ids_y))
    assert c4.hist is None and (c4.sx, c4.sxx, c4.sxy) == (c.sx, c.sxx, c.sxy)


def test_k_range_split_and_reproducibility(ml_nj, sample3000):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample3000
    dx, dy = T1._device_tree(), T2._device_tree()
    K = len(x)
    edges = (np.linspace(x.min(), x.max(), 65), np.linspace(y.min(), y.max(), 33))
    m_all, h_all = dx.compare_triangle_host(dy, ids_x, ids_y, edges=edges)
    m_lo, h_lo = dx.compare_triangle_host(dy, ids_x, ids_y, 0, K // 2, edges=edges)
    m_hi, h_hi = dx.compare_triangle_host(dy, ids_x, ids_y, K // 2, K - K // 2, edges=edges)
    assert np.array_equal(h_lo + h_hi, h_all) and h_all.sum() == K
    full = DistanceComparison.from_moments(m_all, h_all, *edges)
    merged = DistanceComparison.merge(DistanceComparison.from_moments(m_lo, h_lo, *edges),
                                      DistanceComparison.from_moments(m_hi, h_hi, *edges))
    assert merged.n_pairs == full.n_pairs == K and np.array_equal(merged.hist, full.hist)
    for k in ("mean_x", "mean_y", "var_x", "var_y", "cov", "pearson_r"):
        assert _rel(getattr(merged, k), getattr(full, k)) < 1e-12, k
    # two identical calls: identical bits
    m_again, h_again = dx.compare_triangle_host(dy, ids_x, ids_y, edges=edges)
    assert ctypes.string_at(ctypes.addressof(m_again), ctypes.sizeof(m_again)) == ctypes.string_at(ctypes.addressof(m_all), ctypes.sizeof(m_all))
    assert np.array_equal(h_again, h_all)
    m1, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    m2, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    assert bytes(m1) == bytes(m2)


def test_explicit_pairs_of_the_docs_workflow(ml_nj):
    """The 300,000 seeded name pairs of test_docs_correlations_between_ml_and_nj_tree, reduced on the GPU."""
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    idx = np.random.default_rng(11).integers(0, len(leaves1), (300_000, 2))
    px, py = leaves1[idx], nj_of[idx]
    x, y = O1.distances_mt(px, CORES), O2.distances_mt(py, CORES)
    c = T1.compare_distances(T2, pairs=(px, py), bins=(40, 50))
    assert c.n_leaves is None
    assert abs(c.pearson_r - pearsonr(x, y)[0]) < 1e-12
    assert abs(c.pearson_r - 0.969) < 0.0015
    _check_moments(c, x, y)
    assert np.array_equal(c.hist, np.histogram2d(x, y, bins=(40, 50))[0].astype(np.int64))
    # the name form: the same pairs through each tree's leaf names
    A = SuchTree((T1._flat.parent, T1._flat.distance, ["taxon%d" % i for i in range(len(leaves1))]))
    names_b = [None] * len(leaves1)
    rank_b = {int(v): i for i, v in enumerate(np.sort(nj_of))}
    for i, v in enumerate(nj_of):
        names_b[rank_b[int(v)]] = "taxon%d" % i
    B = SuchTree((T2._flat.parent, T2._flat.distance, names_b))
    name_of = list(A.leaves)
    pairs = [(name_of[a], name_of[b]) for a, b in idx[:20_000]]
    cn = A.compare_distances(B, pairs=pairs)
    assert abs(cn.pearson_r - pearsonr(x[:20_000], y[:20_000])[0]) < 1e-12


def test_all_pairs_of_ml_and_nj(ml_nj):
    T1, T2, _, _, leaves1, nj_of = ml_nj
    t0 = time.perf_counter()
    c = T1.compare_distances(T2, leaves=(leaves1, nj_of), bins=64)
    wall = time.perf_counter() - t0
    n = 54327 * 54326 // 2
    assert n == 1_475_684_301
    assert c.n_pairs == n and c.n_leaves == 54327
    assert c.hist.sum() == n                      # range = (min, max): every pair is counted
    print("all pairs of ml vs nj: pearson_r %.6f, %.2f s (two passes)" % (c.pearson_r, wall))
    assert abs(c.pearson_r - 0.969) < 0.0015, c.pearson_r
    assert wall < 30


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
def test_linked_distances_summary(which):
    SLT = _slt(which)
    res = SLT.linked_distances()
    s = SLT.linked_distances_summary(bins=16)
    assert s.n_pairs == res["n_pairs"] and s.n_leaves == SLT.n_links
    r = pearsonr(res["TreeA"], res["TreeB"])[0]
    assert abs(s.pearson_r - r) < 1e-12
    assert np.array_equal(s.hist, np.histogram2d(res["TreeA"], res["TreeB"], 16)[0].astype(np.int64))
    if which == "gopher_louse":
        # the notebook's printed value: linked_distances() itself (float32 sums, as the reference accumulates) lands
        # 4.8e-8 from it, which test_gpu_callers.py::test_config5_linked_distances bounds at 1e-6; the summary equals
        # linked_distances() to 1e-12 above, so the same bar applies here
        assert abs(s.pearson_r - KNOWN["gopher_louse_linked_distances"]["pearson_r"]) < 1e-6


def test_linked_distances_summary_synthetic_and_subset():
    pa, da = synth.balanced_tree(8)
    pb, db = synth.random_binary_tree(5000, seed=3)
    A = SuchTree((pa, da, ["a%d" % i for i in range(256)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(5000)]))
    rows = np.random.default_rng(8).integers(0, 256, 5000)
    mat = np.zeros((256, 5000), dtype=np.int64)
    mat[rows, np.arange(5000)] = 1
    SLT = SuchLinkedTrees(A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves)))
    assert SLT.n_links == 5000
    for step in ("whole", "subset_a"):
        if step == "subset_a":
            SLT.subset_a(int(A.get_children(A.root_node)[0]))
            assert SLT.subset_n_links < 5000
        res = SLT.linked_distances()
        x, y = res["TreeA"], res["TreeB"]
        s = SLT.linked_distances_summary(bins=(32, 48), range=[(x.min(), np.median(x)), (y.min(), y.max())])
        _check_moments(s, x, y)
        want = np.histogram2d(x, y, bins=(32, 48), range=[(x.min(), np.median(x)), (y.min(), y.max())])[0]
        assert np.array_equal(s.hist, want.astype(np.int64))


def test_edge_cases(ml_nj):
    T1, T2, _, _, leaves1, nj_of = ml_nj
    ids = leaves1[:2000]
    c = T1.compare_distances(T1, leaves=(ids, ids), bins=8)      # the same tree twice: one lock, no hang
    assert abs(c.pearson_r - 1.0) < 1e-15 and c.hist.trace() == c.n_pairs
    e = T1.compare_distances(T2, leaves=(leaves1[:1], nj_of[:1]), bins=8, range=[(0, 1), (0, 1)])
    assert e.n_pairs == 0 and np.isnan(e.pearson_r) and np.isnan(e.mean_x) and e.hist.sum() == 0
    with pytest.raises(InvalidNodeError):
        T1.compare_distances(T2, leaves=(np.array([leaves1[0], T1.size + 5]), nj_of[:2]))
    with pytest.raises(InvalidNodeError):
        T1.compare_distances(T2, pairs=(np.array([[leaves1[0], leaves1[1]]]), np.array([[-3, nj_of[0]]])))


def test_trees_on_different_devices_are_refused(ml_nj):
    if _capi.device_count() < 2:
        pytest.skip("one GPU visible: the other-device case needs two")
    T1, T2, _, _, leaves1, nj_of = ml_nj
    other = SuchTree((T2._flat.parent, T2._flat.distance), device=1)
    with pytest.raises(ValueError):
        T1.compare_distances(other, leaves=(leaves1[:10], nj_of[:10]))
