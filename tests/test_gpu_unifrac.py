"""The UniFrac kernels on the GPU: st_unifrac_depths(device = 0) against its host restatement, integer for integer, on the
shapes of tests/test_unifrac_host.py, on both sides of the lane / wave threshold and with more heavy pairs in a chunk than the
wave kernel's fixed grid has waves (its loop's second trip); st_unifrac_host on a golden tree with
an internal node as root; and the facade (SuchTree.unifrac, SuchLinkedTrees.partner_unifrac).  Every comparison of
integers is exact."""
import numpy as np
import pandas as pd
import pytest

import unifrac_cases as uc
from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi

pytestmark = pytest.mark.gpu

LANE_MAX = _capi.UNIFRAC_LANE_MAX


@pytest.fixture(scope="module")
def cases():
    """(d, h, sets, the host restatement's (pd_q, union_q)) per universe size: computed once, never changed."""
    out = {}
    for n in (1, 2, 3, 64, 65, 1000):
        _, _, _, d, h, sets = uc.case(n)
        out[n] = (d, h, sets, _capi.unifrac_depths(d, h, sets, device=-1))
    return out


def _same(got, want, what):
    for name, g, w in (("pd_q", got[0], want[0]), ("union_q", got[1], want[1])):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s: %d of %d %s differ, first at %d: got %d want %d" % (what, len(bad), len(w), name, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_kernels_equal_the_restatement(cases, n):
    d, h, sets, want = cases[n]
    sizes = [len(s) for s in sets]
    if n >= 1000:      # both forms are at work
        assert min(sizes) == 0 and max(sizes) * 2 > LANE_MAX and any(a + b <= LANE_MAX for a in sizes for b in sizes)
    for chunk in (0, 64):
        _same(_capi.unifrac_depths(d, h, sets, device=0, chunk_pairs=chunk), want, "n %d chunk_pairs %d" % (n, chunk))


def test_threshold_chunks_of_one_kind_and_a_range_from_mid_row():
    n = 1000
    _, _, _, d, h, _ = uc.case(n)
    rng = np.random.default_rng(77)
    pick = lambda k: np.sort(rng.choice(n, k, replace=False))      # noqa: E731
    half = LANE_MAX // 2
    # |A| + |B| at the threshold - 1, at it and at + 1, also as PD tasks (2 |A|), with shared positions and without
    edge = [pick(half - 1), pick(half), pick(half), pick(half + 1), np.arange(half), np.arange(half, 2 * half), np.arange(half + 1)]
    total = {len(edge[i]) + len(edge[j]) for i in range(len(edge)) for j in range(i)}
    assert {LANE_MAX - 1, LANE_MAX, LANE_MAX + 1} <= total
    _same(_capi.unifrac_depths(d, h, edge, device=0), _capi.unifrac_depths(d, h, edge, device=-1), "threshold")
    # 13 light sets, then 13 heavy ones: with 64 pairs per chunk the first chunk holds light pairs only (78 pairs among the
    # light sets), the second is mixed, the others hold heavy pairs only; 325 pairs are 6 chunks: both slots of the ring are
    # used three times and the heavy counter is zeroed six times
    sets = [pick(int(k)) for k in rng.integers(0, 11, 13)] + [pick(int(k)) for k in rng.integers(LANE_MAX + 1, LANE_MAX + 200, 13)]
    assert 2 * 10 <= LANE_MAX and LANE_MAX + 200 <= n      # (light with light is a light pair, anything with a heavy set a heavy one)
    want = _capi.unifrac_depths(d, h, sets, device=-1)
    assert len(want[1]) == 325
    _same(_capi.unifrac_depths(d, h, sets, device=0, chunk_pairs=64), want, "light / mixed / heavy chunks")
    _same(_capi.unifrac_depths(d, h, sets, device=0), want, "one chunk")
    mid = 20 * 19 // 2 + 7      # pair (20, 7)
    got = _capi.unifrac_depths(d, h, sets, begin=mid, count=100, device=0, chunk_pairs=64)
    _same(got, (want[0], want[1][mid:mid + 100]), "a range from mid-row")
    # a wave-form set of 1000 positions against a set of one, an empty one and itself
    wide = [np.arange(n), np.array([5]), np.array([], dtype=np.int64), np.arange(n)]
    _same(_capi.unifrac_depths(d, h, wide, device=0), _capi.unifrac_depths(d, h, wide, device=-1), "1000 against 1")


def test_more_heavy_pairs_in_a_chunk_than_the_wave_grid_has_waves():
    """k_unifrac_wave drains a chunk's heavy list with kUnifracWaveBlocks * 4 = 8192 waves: 8385 heavy pairs in one chunk take
    the first 193 waves through `w += waves` once; chunks of 8256 and 129 pairs take two trips and one."""
    n, waves = 600, 2048 * 4      # unifrac_plan.h: kUnifracWaveBlocks workgroups of kUnifracThreads / 64 waves
    _, _, _, d, h, _ = uc.case(n)
    rng = np.random.default_rng(78)
    sets = [np.sort(rng.choice(n, LANE_MAX // 2 + 1, replace=False)) for _ in range(130)]
    pairs = len(sets) * (len(sets) - 1) // 2
    assert pairs == 8385 > waves
    assert all(len(a) + len(b) > LANE_MAX for a in sets for b in sets)      # every pair and every PD task is heavy
    want = _capi.unifrac_depths(d, h, sets, device=-1)
    assert len(want[0]) == 130 and len(want[1]) == pairs
    _same(_capi.unifrac_depths(d, h, sets, device=0), want, "one chunk of 8385 heavy pairs")
    assert waves < 8256 < pairs
    _same(_capi.unifrac_depths(d, h, sets, device=0, chunk_pairs=8256), want, "chunks of 8256 and 129 heavy pairs")


def test_seventeen_table_levels():
    n = 1 << 17
    rng = np.random.default_rng(17)
    d = rng.integers(-2 ** 39, 2 ** 39, n)
    h = rng.integers(-2 ** 39, 2 ** 39, n - 1)
    sets = [np.sort(rng.choice(n, int(k), replace=False)) for k in np.exp(rng.uniform(0, np.log(5000), 34)).astype(int)]
    sets += [np.array([0, n - 1]), np.array([0, n // 2]), np.array([n // 2 - 1, n - 1]), np.arange(0, n, 4099), np.arange(n - 70000, n, 7),
             np.array([0, 1, n - 2, n - 1])]
    assert len(sets) == 40
    _same(_capi.unifrac_depths(d, h, sets, device=0), _capi.unifrac_depths(d, h, sets, device=-1), "n = 2^17")


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links), links


def test_tree_path_with_an_internal_root():
    slt, _ = _slt("fish_worm")
    tb = slt.TreeB
    order = tb._depth_first_leaves()
    leaves = _capi.clade_plan(tb._flat.parent, np.sort(order))
    # the largest clade below the root
    root = max((v for v in range(tb.size) if v != tb.root_node and tb._flat.left[v] != -1), key=lambda v: leaves["count"][v])
    lo, n = int(leaves["begin"][root]), int(leaves["count"][root])
    univ = order[lo:lo + n]
    assert 8 <= n < len(order)
    rng = np.random.default_rng(4)
    sets = [np.sort(rng.choice(n, int(k), replace=False)) for k in rng.integers(0, min(n, 40), 30)] + [np.arange(n), np.array([0, n - 1])]
    dev = tb._device_tree()
    pd_q, union_q, shift, d, h = dev.unifrac_host(root, univ, sets)
    want_d = tb.distances_bulk(np.stack([np.full(n, root), univ], axis=1))
    assert d.dtype == np.float32 and (d.astype(np.float64).view(np.int64) == np.asarray(want_d, dtype=np.float64).view(np.int64)).all()
    mrca = np.array([tb.common_ancestor(int(a), int(b)) for a, b in zip(univ[:-1], univ[1:])], dtype=np.int64)
    want_h = tb.distances_bulk(np.stack([np.full(n - 1, root), mrca], axis=1))
    assert (h.astype(np.float64).view(np.int64) == np.asarray(want_h, dtype=np.float64).view(np.int64)).all()
    d_q, h_q, used = _capi.unifrac_quantise(d, h)
    assert used == shift
    _same((pd_q, union_q), _capi.unifrac_depths(d_q, h_q, sets, device=-1), "tree path")
    for chunk in (1, 7):
        again = dev.unifrac_host(root, univ, sets, chunk_pairs=chunk)
        _same(again[:2], (pd_q, union_q), "tree path, chunk_pairs %d" % chunk)
        assert again[2] == shift
    fixed = dev.unifrac_host(root, univ, sets, begin=10, count=50, shift=shift - 3)
    d_q3, h_q3, _ = _capi.unifrac_quantise(d, h, shift - 3)
    _same(fixed[:2], _capi.unifrac_depths(d_q3, h_q3, sets, begin=10, count=50, device=-1), "tree path, a caller's shift")
    with pytest.raises(ValueError):
        dev.unifrac_host(root, univ, sets, shift=shift + 1)      # the largest depth would reach 2^40
    for bad_univ, bad_root in ((np.append(univ[:-1], tb.size), root), (univ, tb.size), (np.append(univ[:-1], -1), root)):
        with pytest.raises(_capi.InvalidNodeError):      # checked on the host, before anything is launched
            dev.unifrac_host(bad_root, bad_univ, sets)


def _state(slt):
    return (slt.subset_a_root, slt.subset_b_root, slt.subset_a_size, slt.subset_b_size, slt.subset_a_leafs.tolist(), slt.subset_b_leafs.tolist(),
            slt.subset_rows.tolist(), slt.subset_columns.tolist(), slt.linklist.tolist(), slt._seed)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("of", ["A", "B"])
def test_facade(which, of):
    slt, links = _slt(which)
    before = _state(slt)
    res = slt.partner_unifrac(of=of)
    assert _state(slt) == before
    # the rows are partner_dispersion's for the same bounds
    ref = slt.partner_dispersion(of=of, permutations=0, seed=1, min_partners=1)
    assert res.names == ref.names and res.leaves.tolist() == ref.leaves.tolist() and len(res) == len(ref) > 2
    own, partner = (slt.TreeA, slt.TreeB) if of == "A" else (slt.TreeB, slt.TreeA)
    assert res.root == partner.root_node and res.count == len(res) * (len(res) - 1) // 2
    u = res.unifrac
    assert (res.pd > 0).all() and ((u >= 0) & (u <= 1)).all() and ((res.phylosor >= 0) & (res.phylosor <= 1)).all()
    M = res.matrix()
    assert M.shape == (len(res), len(res)) and (M == M.T).all() and not M.diagonal().any()
    # two leaves with identical partner sets are at distance 0
    col = 1 if of == "A" else 0
    partners = [frozenset(slt.linklist[slt.linklist[:, col] == leaf, 1 - col].tolist()) for leaf in res.leaves]
    same = np.array([partners[i] == partners[j] for i in range(len(res)) for j in range(i)])
    assert (u[same] == 0).all() and (res.phylosor[same] == 1).all()
    # SuchTree.unifrac on the same sets, by name
    names = partner.leaf_nodes
    direct = partner.unifrac([[names[int(b)] for b in sorted(p)] for p in partners])
    assert (direct.pd_q == res.pd_q).all() and (direct.union_q == res.union_q).all() and direct.shift == res.shift
    # a fixed shift makes two range calls agree with one whole call
    cut = res.count // 3
    a = slt.partner_unifrac(of=of, begin=0, count=cut, shift=res.shift)
    b = slt.partner_unifrac(of=of, begin=cut, shift=res.shift)
    assert (np.concatenate([a.union_q, b.union_q]) == res.union_q).all() and (a.pd_q == res.pd_q).all() and (b.pd_q == res.pd_q).all()
    assert b.pair(0) == res.pair(cut) and len(res.to_dataframe()) == res.count
    with pytest.raises(ValueError):
        a.matrix()
    names = partner.leaf_nodes
    twice = partner.unifrac([[names[int(b)] for b in sorted(p)] for p in (partners[0], partners[1], partners[0])], shift=res.shift)
    assert twice.unifrac[1] == 0 and twice.union_q[1] == res.pd_q[0] and twice.unifrac[0] == u[0] == twice.unifrac[2]
    few = slt.partner_unifrac(of=of, min_partners=2, max_partners=3, shift=res.shift)
    picked = [i for i, p in enumerate(partners) if 2 <= len(p) <= 3]
    assert few.leaves.tolist() == res.leaves[picked].tolist() and (few.pd_q == res.pd_q[picked]).all()


def test_facade_under_a_subset():
    slt, _ = _slt("gopher_louse")
    leaves = SuchLinkedTrees._leaf_counts(slt.TreeB)
    node = max((int(v) for v in slt.TreeB.internal_nodes if int(v) != slt.TreeB.root_node), key=lambda v: leaves[v])
    slt.subset_b(node)
    before = _state(slt)
    res = slt.partner_unifrac(of="A")
    assert _state(slt) == before and res.root == node == slt.subset_b_root and len(res) > 1
    ref = slt.partner_dispersion(of="A", permutations=0, seed=1, min_partners=1)
    assert res.names == ref.names
    # SuchTree.unifrac on the same sets with the subset root as root
    names = slt.TreeB.leaf_nodes
    sets = [[names[int(b)] for b in slt.linklist[slt.linklist[:, 1] == leaf, 0]] for leaf in res.leaves]
    below = slt.TreeB.unifrac(sets, root=node)
    assert below.shift == res.shift and (below.pd_q == res.pd_q).all() and (below.union_q == res.union_q).all()
    # from the tree's root every set pays the stem between the two roots as well
    whole = slt.TreeB.unifrac(sets)
    stem = slt.TreeB.distance(slt.TreeB.root_node, node)
    assert stem > 0 and np.allclose(whole.pd - res.pd, stem, rtol=0, atol=1e-5 * whole.pd.max())
