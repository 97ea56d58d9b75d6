"""Exact Kendall tau-b on the GPU (compare_distances(kendall=True), linked_distances_summary(kendall=True), C ABI
st_compare_*_kendall_host, st_kendall_arrays_host): the integer counts against st_kendall_host on the oracle's float32
distances -- equal, not close -- and kendall_tau against scipy; tie runs that span hundreds of blocks of sorted keys, so that
a thread of k_kendall_tie_carry owns two or three blocks and carries a run start across blocks that hold none."""
import dataclasses
import math
import os

import numpy as np
import pandas as pd
import pytest
from scipy.stats import kendalltau

from conftest import golden_path
from kendall_reference import heavy_columns, tie_sum
from oracle.oracle import OracleTree
from rank_reference import bit_reverse
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.compare import kendall_fields
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu
CORES = len(os.sched_getaffinity(0))
KENDALL_FIELDS = ("kendall_tau", "concordant", "discordant", "ties_x", "ties_y", "ties_xy")
T = _capi.KENDALL_TILE
SIZES = (0, 1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T, 5 * T + 7)


def _tri_pairs(ids):
    rows, cols = np.tril_indices(len(ids), -1)
    return np.stack([ids[cols], ids[rows]], axis=1).astype(np.int64)


def _f32(d):
    f = d.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), d, equal_nan=True)      # the oracle's distances are float32 sums
    return f


def _same_counts(got, want):
    assert got.as_tuple() == want.as_tuple(), (got.as_tuple(), want.as_tuple())


def _same_as_host(c, x, y, scipy=True):
    """The Kendall fields of DistanceComparison c against st_kendall_host and scipy on the float32 columns x, y."""
    want = _capi.kendall_host(x, y)
    assert (c.concordant, c.discordant, c.ties_x, c.ties_y, c.ties_xy) == (want.concordant, want.discordant, want.ties_x, want.ties_y, want.ties_xy)
    assert c.kendall_tau == kendall_fields(want)["kendall_tau"] or (math.isnan(c.kendall_tau) and math.isnan(kendall_fields(want)["kendall_tau"]))
    if scipy:
        tau = kendalltau(x, y)[0]
        print("kendall_tau %.17g, scipy %.17g, difference %.3g" % (c.kendall_tau, tau, c.kendall_tau - tau))
        assert abs(c.kendall_tau - tau) < 1e-12
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
    c = T1.compare_distances(T2, leaves=(ids_x, ids_y), kendall=True)
    _same_as_host(c, x, y)
    plain = T1.compare_distances(T2, leaves=(ids_x, ids_y))
    for f in dataclasses.fields(c):
        if f.name in KENDALL_FIELDS:
            assert getattr(plain, f.name) is None
        else:      # every other field: the same bits
            a, b = getattr(c, f.name), getattr(plain, f.name)
            assert a is b is None or a == b or (np.isnan(a) and np.isnan(b)), f.name
    # with a histogram and with ranks: those calls as they are without kendall, the counts beside them
    counts = tuple(getattr(c, k) for k in KENDALL_FIELDS)
    h = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=16, kendall=True)
    h0 = T1.compare_distances(T2, leaves=(ids_x, ids_y), bins=16)
    assert np.array_equal(h.hist, h0.hist) and (h.sx, h.sxx, h.sxy, h.pearson_r) == (h0.sx, h0.sxx, h0.sxy, h0.pearson_r)
    assert tuple(getattr(h, k) for k in KENDALL_FIELDS) == counts and h.spearman_r is None
    s = T1.compare_distances(T2, leaves=(ids_x, ids_y), spearman=True, kendall=True)
    s0 = T1.compare_distances(T2, leaves=(ids_x, ids_y), spearman=True)
    for f in dataclasses.fields(s):
        if f.name in KENDALL_FIELDS:
            continue
        a, b = getattr(s, f.name), getattr(s0, f.name)
        assert a is b is None or a == b or (np.isnan(a) and np.isnan(b)), f.name
    assert tuple(getattr(s, k) for k in KENDALL_FIELDS) == counts and s.rank_sxy is not None


def test_chunks_and_repeats_return_the_same_bytes(ml_nj, sample600):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample600
    dx, dy = T1._device_tree(), T2._device_tree()
    assert len(x) == 179_700                      # 21 chunks of 8192 and a tail, 2 of 65536 and a tail
    want = _capi.kendall_host(x, y)
    m0, _ = dx.compare_triangle_host(dy, ids_x, ids_y)
    seen = []
    for chunk in (8192, 65536, 0, 0):
        m, c = dx.compare_triangle_kendall_host(dy, ids_x, ids_y, chunk_pairs=chunk)
        _same_counts(c, want)
        assert bytes(m) == bytes(m0)              # the moments of the existing call, whatever the chunk
        seen.append(bytes(c))
    assert len(set(seen)) == 1
    for bad in (-8192, 100, 8191):
        with pytest.raises(ValueError):
            dx.compare_triangle_kendall_host(dy, ids_x, ids_y, chunk_pairs=bad)


def test_sub_ranges_agree_with_the_host_on_the_slice(ml_nj, sample600):
    T1, T2 = ml_nj[:2]
    ids_x, ids_y, x, y = sample600
    dx, dy = T1._device_tree(), T2._device_tree()
    K = len(x)
    for k0, kc, chunk in ((0, K // 3, 0), (K // 3, K - K // 3, 16384), (12345, 8192 + 3, 8192), (K - 1, 1, 0), (7, 2, 0), (99, T + 1, 0)):
        m, c = dx.compare_triangle_kendall_host(dy, ids_x, ids_y, k0, kc, chunk_pairs=chunk)
        _same_counts(c, _capi.kendall_host(x[k0:k0 + kc], y[k0:k0 + kc]))
        assert bytes(m) == bytes(dx.compare_triangle_host(dy, ids_x, ids_y, k0, kc)[0])
    m, c = dx.compare_triangle_kendall_host(dy, ids_x, ids_y, 5, 0)
    assert m.n == 0 and c.as_tuple() == (0, 0, 0, 0, 0, 0)


def test_explicit_pairs_with_repeated_pairs_and_internal_nodes(ml_nj):
    T1, T2, O1, O2, leaves1, nj_of = ml_nj
    rng = np.random.default_rng(5)
    px = rng.integers(0, T1.size, (40_000, 2))               # any node, internal ones included
    py = rng.integers(0, T2.size, (40_000, 2))
    px[:500, 1] = px[:500, 0]                                # (a, a)
    py[250:750, 1] = py[250:750, 0]
    px[20_000:30_000], py[20_000:30_000] = px[5_000:15_000], py[5_000:15_000]      # repeated pairs: joint ties
    x, y = _f32(O1.distances_mt(px, CORES)), _f32(O2.distances_mt(py, CORES))
    c = T1.compare_distances(T2, pairs=(px, py), kendall=True)
    want = _same_as_host(c, x, y)
    assert want.ties_xy >= 10_000
    dx, dy = T1._device_tree(), T2._device_tree()
    m0, _ = dx.compare_pairs_host(dy, px, py)
    for chunk in (8192, 0):
        m, got = dx.compare_pairs_kendall_host(dy, px, py, chunk_pairs=chunk)
        _same_counts(got, want)
        assert bytes(m) == bytes(m0)


@pytest.mark.parametrize("n", SIZES)
def test_arrays_against_the_host_at_the_tile_edges(n):
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal(n).astype(np.float32)
    y = (0.5 * x + rng.standard_normal(n)).astype(np.float32)
    _same_counts(_capi.kendall_arrays_host(x, y), _capi.kendall_host(x, y))
    hx, hy = heavy_columns(n, 200 + n, values=5)             # tie groups that span tiles and runs
    _same_counts(_capi.kendall_arrays_host(hx, hy), _capi.kendall_host(hx, hy))


@pytest.mark.parametrize("blocks, per", [(300, 2), (600, 3)])
def test_tie_runs_over_more_blocks_than_the_carry_kernel_has_threads(blocks, per):
    """k_kendall_tie_carry: 256 threads own per = ceil(n_blocks / 256) consecutive blocks each.  Two tie groups in x, two
    thirds and one third of the keys: all but two blocks of a column's sorted keys hold no run start of x, so the running
    maximum of a thread's last loop has to pass an earlier block's start on."""
    n = blocks * T + (5 if per == 2 else 1)
    n_blocks = -(-n // T)
    assert n_blocks == blocks + 1 and -(-n_blocks // 256) == per
    x, y = heavy_columns(n, 300 + blocks, values=2)
    groups = np.unique(x, return_counts=True)[1]
    assert len(groups) == 2 and groups.min() > 64 * T      # (-0.0 and +0.0 are one group)
    want = _capi.kendall_host(x, y)
    got = _capi.kendall_arrays_host(x, y)
    _same_counts(got, want)
    assert (got.ties_x, got.ties_y) == (tie_sum(x), tie_sum(y))


def test_arrays_reversed_equal_zeros_infinities_and_nan():
    n = 200_000
    x = np.arange(n, dtype=np.float32)
    c = _capi.kendall_arrays_host(x, x[::-1].copy())
    assert c.as_tuple() == (n, 0, 19_999_900_000, 0, 0, 0) and kendall_fields(c)["kendall_tau"] == -1.0
    same = _capi.kendall_arrays_host(x, x)
    assert same.as_tuple() == (n, 0, 0, 0, 0, 0) and kendall_fields(same)["kendall_tau"] == 1.0
    const = np.full(3 * T + 5, 2.5, np.float32)
    n0 = len(const) * (len(const) - 1) // 2
    for a, b in ((const, const), (const, x[:len(const)]), (x[:len(const)], const)):
        c = _capi.kendall_arrays_host(a, b)
        _same_counts(c, _capi.kendall_host(a, b))
        assert c.discordant == 0 and (c.ties_x == n0 or c.ties_y == n0) and math.isnan(kendall_fields(c)["kendall_tau"])
    rng = np.random.default_rng(7)
    pool = np.float32([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 3.0e-45, -3.0e-45])
    zx, zy = pool[rng.integers(0, 8, 3 * T)], pool[rng.integers(0, 8, 3 * T)]
    c = _capi.kendall_arrays_host(zx, zy)
    _same_counts(c, _capi.kendall_host(zx, zy))
    assert abs(kendall_fields(c)["kendall_tau"] - kendalltau(zx, zy)[0]) < 1e-12
    bad = zx.copy()
    bad[T + 3] = np.nan
    for a, b in ((bad, zy), (zx, bad)):
        assert _capi.kendall_arrays_host(a, b).as_tuple() == (3 * T, 1, 0, 0, 0, 0)
        assert _capi.kendall_host(a, b).as_tuple() == (3 * T, 1, 0, 0, 0, 0)


def test_perfect_tree_against_itself_and_bit_reversed():
    L = 10
    parent, distance = synth.balanced_tree(L)
    distance = np.where(parent < 0, distance, np.float32(1.0)).astype(np.float32)
    X, O = SuchTree((parent, distance)), OracleTree(parent, distance)
    ids = 2 * np.arange(1 << L, dtype=np.int64)              # leaf k has id 2 k
    x = _f32(O.distances_mt(_tri_pairs(ids), CORES))
    assert len(x) == 523_776
    c = X.compare_distances(X, leaves=(ids, ids), kendall=True)
    _, t = np.unique(x, return_counts=True)
    ties = sum(int(v) * (int(v) - 1) // 2 for v in t)
    assert c.discordant == 0 and c.ties_x == c.ties_y == c.ties_xy == ties and c.kendall_tau == 1.0
    assert c.concordant == 523_776 * 523_775 // 2 - ties
    rev = 2 * bit_reverse(np.arange(1 << L), L)
    y = _f32(O.distances_mt(_tri_pairs(rev), CORES))
    _same_as_host(X.compare_distances(X, leaves=(ids, rev), kendall=True), x, y)


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
def test_linked_distances_summary_kendall(which):
    SLT = _slt(which)
    res = SLT.linked_distances()
    s = SLT.linked_distances_summary(kendall=True)
    assert s.n_pairs == res["n_pairs"]
    _same_as_host(s, _f32(np.asarray(res["TreeA"])), _f32(np.asarray(res["TreeB"])))
    plain = SLT.linked_distances_summary()
    assert plain.kendall_tau is None and (plain.sx, plain.sxx, plain.sxy, plain.pearson_r) == (s.sx, s.sxx, s.sxy, s.pearson_r)
    sb = SLT.linked_distances_summary(bins=8, spearman=True, kendall=True)
    assert sb.hist.sum() == s.n_pairs and (sb.discordant, sb.kendall_tau) == (s.discordant, s.kendall_tau) and sb.spearman_r is not None
