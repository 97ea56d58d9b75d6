"""Hommola's permutation test for every clade in one GPU pass (SuchLinkedTrees.hommola_by_clade, C ABI
st_hommola_clades_host).  The yardsticks are the existing st_compare_rows_host -- on the id rows that the numpy
restatement of the definitions gives (tests/hommola_clade_reference.py), bit for bit -- and hommola_cospeciation.  Universes
go up to 4096 leaves (the default cap) and to 8200 (k_hommola_relabel<1024> above 8192 positions, 128 KiB of sort keys)."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path

import hommola_clade_reference as ref
from suchtree_amd import SuchTree, _capi, compare, synth
from suchtree_amd.compare import row_stats, _SUMS
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu


def _named(tree, prefix):
    parent, dist = tree
    return SuchTree((parent, dist, ["%s%d" % (prefix, i) for i in range((len(parent) + 1) // 2)]))


def _system(tree_a, tree_b, links_ab):
    """SuchLinkedTrees over two synthetic trees; links_ab: (TreeA leaf id, TreeB leaf id) pairs."""
    A, B = _named(tree_a, "a"), _named(tree_b, "b")
    names_a, names_b = list(A.leaves), list(B.leaves)
    row = {int(A.leaves[k]): i for i, k in enumerate(names_a)}
    col = {int(B.leaves[k]): i for i, k in enumerate(names_b)}
    mat = np.zeros((len(names_a), len(names_b)), dtype=np.int64)
    for a, b in links_ab:
        mat[row[int(a)], col[int(b)]] = 1
    return SuchLinkedTrees(A, B, pd.DataFrame(mat, index=names_a, columns=names_b))


def _leaf_ids(T):
    return np.sort(np.asarray(T.leaf_node_ids, dtype=np.int64))


def _clades(layout, nodes):
    c = np.zeros(len(nodes), dtype=_capi.HOMMOLA_CLADE)
    for i, v in enumerate(nodes):
        lo, n = layout.links(v)
        c[i] = (v, layout.leaf_begin[v], layout.leaf_count[v], lo, n, 0)
    return c


def _inner_nodes(T, layout, min_links=3, max_leaves=None):
    left = np.asarray(T._flat.left)
    return [int(v) for v in np.flatnonzero(left != -1)
            if layout.links(v)[1] >= min_links and (max_leaves is None or layout.leaf_count[v] <= max_leaves)]


def _low_level(S, layout, nodes, permutations, seed, chunk_blocks=0):
    """st_hommola_clades_host with TreeB as the clade tree: (clades, permutations + 1) records, x = TreeA."""
    return S.TreeA._device_tree().hommola_clades_host(S.TreeB._device_tree(), layout.univ_o, layout.univ_c, layout.pos_o, layout.pos_c,
                                                      _clades(layout, nodes), permutations, seed, chunk_blocks)


def _check_rows(S, layout, nodes, got, permutations, seed):
    """every row of every clade against st_compare_rows_host on the restated ids, bit for bit"""
    dA, dB = S.TreeA._device_tree(), S.TreeB._device_tree()
    for i, v in enumerate(nodes):
        ids_o, ids_c = layout.rows(v, permutations, seed)
        want = dA.compare_rows_host(dB, ids_o, ids_c)
        assert got[i].tobytes() == want.tobytes(), (v, layout.links(v))


def _state(S):
    return (S.subset_a_root, S.subset_b_root, S.subset_a_size, S.subset_b_size, S.subset_n_links,
            S.subset_a_leafs.copy(), S.subset_b_leafs.copy(), S.linklist.copy(), S._seed)


def _same_state(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.fixture(scope="module")
def caterpillar():
    """TreeB = a caterpillar of 184 leaves with exactly one link per leaf, TreeA = 40 leaves of which 5 stay unlinked."""
    ta, tb = synth.random_binary_tree(40, seed=3), synth.caterpillar_tree(184)
    rng = np.random.default_rng(11)
    a_leaves = np.arange(40, dtype=np.int64) * 2
    used = rng.permutation(a_leaves)[:35]
    links = [(int(rng.choice(used)), int(b)) for b in np.arange(184, dtype=np.int64) * 2]
    S = _system(ta, tb, links)
    # links in rank order: any order will do for the C call; one link per clade leaf leaves no ties
    ids_c = np.array([b for _, b in links], dtype=np.int64)
    ids_o = np.array([a for a, _ in links], dtype=np.int64)
    return S, ref.Layout(S.TreeB._flat.parent, S.TreeA._flat.parent, ids_c, ids_o)


def test_edges_of_the_order_rule(caterpillar):
    """Clades of every link count 3..184: 11 / 12 links (55 / 66 pairs: one lane / one wave), 128 / 129 / 130 links (one
    block; a second block of 64 pairs by lane 0; one of 193 pairs by a wave), 182 links (three blocks)."""
    S, layout = caterpillar
    nodes = _inner_nodes(S.TreeB, layout)
    counts = sorted(layout.links(v)[1] for v in nodes)
    assert counts == list(range(3, 185))
    got = _low_level(S, layout, nodes, 3, 2024)
    assert got.shape == (len(nodes), 4)
    assert np.array_equal(got["n"][:, 0], [c * (c - 1) // 2 for c in (layout.links(v)[1] for v in nodes)])
    _check_rows(S, layout, nodes, got, 3, 2024)
    # the facade reduces the same records
    res = S.hommola_by_clade(permutations=3, seed=2024, keep_stats=True, max_leaves=184)
    assert sorted(res.nodes.tolist()) == sorted(nodes) and res.skipped_nodes.size == 0
    at = {v: i for i, v in enumerate(nodes)}
    r = row_stats(got["n"], *(got[k] for k in _SUMS))[5]
    for i, v in enumerate(res.nodes.tolist()):
        # (the observed r takes every pair in rank order, row 0 in layout order: float32 distances a few ulps apart, 2^-24 each)
        assert abs(res.corr_coeff[i] - r[at[v], 0]) < 1e-5 and res.perm_stats[i].tobytes() == r[at[v], 1:].tobytes()
        assert res.n_links[i] == layout.links(v)[1] and res.n_leaves[i] == layout.leaf_count[v]
        assert res.n_ge[i] == np.count_nonzero(r[at[v], 1:] >= res.corr_coeff[i])
        assert res.p_value[i] == (res.n_ge[i] + 1) / 4
    one = res.result(res.nodes[5])
    assert one.corr_coeff == res.corr_coeff[5] and one.perm_stats.tobytes() == res.perm_stats[5].tobytes()
    assert one.observed.pearson_r == one.corr_coeff and one.n_links == res.n_links[5] and one.seed == 2024
    df = res.to_dataframe()
    assert list(df.columns[:5]) == ["name", "n_links", "n_leafs", "r", "p"] and len(df) == len(res)


@pytest.mark.parametrize("links, chunk_blocks, permutations", [(182, 1, 0), (182, 1, 1), (182, 2, 0), (130, 3, 1)])
def test_drain_order_of_the_last_chunks(caterpillar, links, chunk_blocks, permutations):
    """A row's pieces are merged in block order also when its blocks straddle the last chunks, whose two read-back slots
    are drained after the loop, the older one first -- at both parities of the chunk count.  182 links are 16471 pairs,
    three blocks per row: chunks of 1 + 1 + 1 blocks (odd), of 1 x 6 with one permutation (even), of 2 + 1; 130 links
    are two blocks per row: with one permutation chunks of 3 + 1, row 1 across the cut (tests/emu/sanitize_hommola.cpp
    checks these cuts on the host).  The yardstick reads every row's pieces back in one chunk: no drain order in it."""
    S, layout = caterpillar
    node = next(v for v in _inner_nodes(S.TreeB, layout) if layout.links(v)[1] == links)
    got = _low_level(S, layout, [node], permutations, 2024, chunk_blocks)
    assert got.shape == (1, permutations + 1) and np.all(got["n"] == links * (links - 1) // 2)
    _check_rows(S, layout, [node], got, permutations, 2024)


@pytest.fixture(scope="module")
def nested():
    """TreeB = a random tree of 300 leaves, 400 random links: several links share a leaf, some leaves have none."""
    ta, tb = synth.random_binary_tree(40, seed=5), synth.random_binary_tree(300, seed=6)
    rng = np.random.default_rng(12)
    pairs = sorted({(int(a), int(b)) for a, b in zip(rng.integers(0, 40, 400) * 2, rng.integers(0, 300, 400) * 2)}, key=lambda t: (t[1], t[0]))
    S = _system(ta, tb, pairs)
    ids_c = np.array([b for _, b in pairs], dtype=np.int64)
    ids_o = np.array([a for a, _ in pairs], dtype=np.int64)
    return S, ref.Layout(S.TreeB._flat.parent, S.TreeA._flat.parent, ids_c, ids_o)


def test_nesting_and_matrices(nested):
    S, layout = nested
    assert np.any(np.diff(layout.pos_c) == 0) and len(np.unique(layout.pos_c)) < 300
    # the C call against st_compare_rows_host, for all clades at once and for caps that change the maximal ranges
    full = None
    for cap in (300, 64, 8):
        nodes = _inner_nodes(S.TreeB, layout, max_leaves=cap)
        got = _low_level(S, layout, nodes, 2, 7)
        if full is None:
            full = dict(zip(nodes, (g.tobytes() for g in got)))
            _check_rows(S, layout, nodes[::7], got[::7], 2, 7)
        for v, g in zip(nodes, got):
            assert g.tobytes() == full[v], (cap, v)
    # the facade: rows of evaluated clades identical across the caps, skipped_nodes exact
    before = _state(S)
    want = S.hommola_by_clade(permutations=5, seed=9, keep_stats=True, max_leaves=300)
    assert want.skipped_nodes.size == 0 and len(want) > 100
    row = {int(v): i for i, v in enumerate(want.nodes)}
    for cap in (64, 8):
        res = S.hommola_by_clade(permutations=5, seed=9, keep_stats=True, max_leaves=cap)
        assert res.skipped_nodes.tolist() == [int(v) for v, n in zip(want.nodes, want.n_leaves) if n > cap]
        assert res.nodes.tolist() == [int(v) for v, n in zip(want.nodes, want.n_leaves) if n <= cap] and len(res) > 0
        idx = [row[int(v)] for v in res.nodes]
        assert res.corr_coeff.tobytes() == want.corr_coeff[idx].tobytes() and res.perm_stats.tobytes() == want.perm_stats[idx].tobytes()
        assert np.array_equal(res.n_ge, want.n_ge[idx]) and np.array_equal(res.n_nan, want.n_nan[idx])
    # nodes= of a single deep clade: that clade's row of the full run
    deep = int(want.nodes[np.argmin(np.where(want.n_leaves >= 5, want.n_leaves, 10 ** 6))])
    one = S.hommola_by_clade(permutations=5, seed=9, keep_stats=True, nodes=[deep])
    assert one.nodes.tolist() == [deep] and one.corr_coeff[0] == want.corr_coeff[row[deep]]
    assert one.perm_stats.tobytes() == want.perm_stats[row[deep]].tobytes()
    # the prefix property, and another seed gives other permutations
    more = S.hommola_by_clade(permutations=8, seed=9, keep_stats=True, nodes=[deep])
    assert more.perm_stats[:, :5].tobytes() == one.perm_stats.tobytes()
    assert S.hommola_by_clade(permutations=5, seed=10, keep_stats=True, nodes=[deep]).perm_stats.tobytes() != one.perm_stats.tobytes()
    assert _same_state(before, _state(S))
    drawn = S.hommola_by_clade(permutations=1, nodes=[deep])
    assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 1 << 64 and drawn.perm_stats is None


def test_chunking_and_grouping(nested, monkeypatch):
    S, layout = nested
    nodes = _inner_nodes(S.TreeB, layout)
    want = _low_level(S, layout, nodes, 2, 7, 0).tobytes()
    for chunk_blocks in (1, 2, 7):
        assert _low_level(S, layout, nodes, 2, 7, chunk_blocks).tobytes() == want, chunk_blocks
    whole = S.hommola_by_clade(permutations=5, seed=9, keep_stats=True, max_leaves=64)
    plain = S.hommola_by_clade(permutations=5, seed=9, max_leaves=64)
    assert plain.perm_stats is None and np.array_equal(plain.n_ge, whole.n_ge) and np.array_equal(plain.n_nan, whole.n_nan)
    assert plain.corr_coeff.tobytes() == whole.corr_coeff.tobytes() and plain.p_value.tobytes() == whole.p_value.tobytes()
    for rows in (1, 50, 1000):      # groups of whole maximal clades, forced small
        monkeypatch.setattr(SuchLinkedTrees, "_HOMMOLA_GROUP_ROWS", rows)
        for chunk_blocks in (0, 2):
            res = S.hommola_by_clade(permutations=5, seed=9, keep_stats=True, max_leaves=64, chunk_blocks=chunk_blocks)
            assert res.nodes.tolist() == whole.nodes.tolist() and res.corr_coeff.tobytes() == whole.corr_coeff.tobytes()
            assert res.perm_stats.tobytes() == whole.perm_stats.tobytes() and np.array_equal(res.n_ge, whole.n_ge)


def test_largest_universe_of_the_default_cap():
    """4096 leaves under the root (the default max_leaves): the 1024-lane sort of 32 KiB of keys, one 64 MiB matrix."""
    ta, tb = synth.random_binary_tree(40, seed=5), synth.balanced_tree(12)
    rng = np.random.default_rng(13)
    pairs = sorted(zip((rng.integers(0, 40, 150) * 2).tolist(), (rng.choice(4096, 150, replace=False) * 2).tolist()), key=lambda t: t[1])
    S = _system(ta, tb, pairs)
    layout = ref.Layout(S.TreeB._flat.parent, S.TreeA._flat.parent, np.array([b for _, b in pairs]), np.array([a for a, _ in pairs]))
    root = int(S.TreeB.root_node)
    got = _low_level(S, layout, [root], 5, 31)
    _check_rows(S, layout, [root], got, 5, 31)
    res = S.hommola_by_clade(permutations=5, seed=31, keep_stats=True, nodes=[root])      # (no two links on one leaf: the same layout)
    r = row_stats(got["n"], *(got[k] for k in _SUMS))[5]
    assert res.n_leaves.tolist() == [4096] and abs(res.corr_coeff[0] - r[0, 0]) < 1e-5 and res.perm_stats[0].tobytes() == r[0, 1:].tobytes()


def test_universe_above_8192_leaves():
    """8200 leaves under the root of a random tree: the relabelling sort with more than 8 keys per lane."""
    ta, tb = synth.random_binary_tree(40, seed=5), synth.random_binary_tree(8200, seed=7)
    rng = np.random.default_rng(14)
    pairs = sorted(zip((rng.integers(0, 40, 150) * 2).tolist(), (rng.choice(8200, 150, replace=False) * 2).tolist()), key=lambda t: t[1])
    S = _system(ta, tb, pairs)
    layout = ref.Layout(S.TreeB._flat.parent, S.TreeA._flat.parent, np.array([b for _, b in pairs]), np.array([a for a, _ in pairs]))
    root = int(S.TreeB.root_node)
    assert layout.leaf_count[root] == 8200 > 8192 and layout.links(root)[1] == 150
    got = _low_level(S, layout, [root], 2, 32)
    assert got.shape == (1, 3)
    _check_rows(S, layout, [root], got, 2, 32)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 16383, 16384])
def test_device_permutation_equals_the_host(n):
    for seed, node, p, side in ((0, 0, 1, 0), (2024, 7, 999, 1), ((1 << 64) - 1, 123456, 3, 0)):
        assert np.array_equal(compare.hommola_permutation(seed, node, p, side, n, device=0), compare.hommola_permutation(seed, node, p, side, n))
    assert np.array_equal(compare.hommola_permutation(1, 1, 0, 0, n, device=0), np.arange(n))


def _fixture(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("tree", ["B", "A"])
def test_fixtures_against_the_per_clade_loop(which, tree):
    S = _fixture(which)
    before = _state(S)
    res = S.hommola_by_clade(tree=tree, permutations=99, seed=4)
    assert _same_state(before, _state(S))
    summary = S.linked_distances_by_clade(tree=tree, min_leaves=3, min_links=3)
    assert res.nodes.tolist() == summary.nodes.tolist() and len(res) > 0
    assert np.array_equal(res.n_links, summary.n_links) and np.array_equal(res.n_leaves, summary.n_leaves)
    assert res.permutations == 99 and res.seed == 4 and res.tree == tree and res.perm_stats is None
    for i, v in enumerate(res.nodes.tolist()):
        (S.subset_b if tree == "B" else S.subset_a)(v)
        want = S.hommola_cospeciation(0).corr_coeff
        assert (np.isnan(want) and np.isnan(res.corr_coeff[i])) or abs(res.corr_coeff[i] - want) < 1e-12, (v, res.corr_coeff[i], want)
        assert S.subset_n_links == res.n_links[i]
    ok = ~np.isnan(res.corr_coeff)
    assert np.all((res.p_value[ok] >= 1 / 100) & (res.p_value[ok] <= 1)) and np.all(res.n_ge + res.n_nan <= 99)
    assert np.array_equal(res.p_value[ok], (res.n_ge[ok] + 1) / 100)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_distribution_against_numpy_draws(seed):
    """Two-sample Kolmogorov-Smirnov distance between the permuted r of this path and of hommola_cospeciation's numpy
    draws, 9999 each, on the gopher_louse root: below 1.95 sqrt(2 / 9999) = 0.0276 (alpha = 0.001).  (A float64
    restatement gave 0.010 to 0.016; p-values cannot tell the two apart here: both sit at 1 / (P + 1).)"""
    S = _fixture("gopher_louse")
    root = int(S.TreeB.root_node)
    S.subset_b(root)      # (the same links in the order subset_b gives them: the order both observed r follow)
    mine = S.hommola_by_clade(permutations=9999, seed=seed, keep_stats=True, nodes=[root], max_leaves=16384)
    assert mine.nodes.tolist() == [root]
    theirs = S.hommola_cospeciation(9999, seed=seed)
    assert abs(mine.corr_coeff[0] - theirs.corr_coeff) < 1e-12
    a, b = np.sort(mine.perm_stats[0]), np.sort(theirs.perm_stats)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    grid = np.concatenate([a, b])
    ks = float(np.max(np.abs(np.searchsorted(a, grid, side="right") / len(a) - np.searchsorted(b, grid, side="right") / len(b))))
    print("KS distance, seed", seed, ks)
    assert ks < 1.95 * np.sqrt(2 / 9999)


def test_nan_rows():
    """every link on one TreeA leaf: x is constant, r is NaN"""
    ta, tb = synth.balanced_tree(4), synth.balanced_tree(5)
    S = _system(ta, tb, [(6, int(b)) for b in np.arange(32) * 2])
    res = S.hommola_by_clade(permutations=20, seed=1, keep_stats=True)
    assert len(res) == 15      # (the inner nodes of 4, 8, 16 and 32 leaves)
    assert np.all(np.isnan(res.corr_coeff)) and np.all(np.isnan(res.p_value)) and np.all(res.n_ge == 0)
    assert np.all(res.n_nan == 20) and np.all(np.isnan(res.perm_stats))


def test_errors():
    ta, tb = synth.balanced_tree(4), synth.balanced_tree(5)
    S = _system(ta, tb, [(int(a), int(b)) for a, b in zip(np.arange(32) % 16 * 2, np.arange(32) * 2)])
    for kw in ({"tree": "C"}, {"permutations": -1}, {"permutations": 1.5}, {"max_leaves": 16385}, {"max_leaves": -1}):
        with pytest.raises(ValueError):
            S.hommola_by_clade(**kw)
    leaf = int(_leaf_ids(S.TreeB)[0])
    for bad in ([leaf], [S.TreeB.size], [-1]):
        with pytest.raises(ValueError, match="not an internal node"):
            S.hommola_by_clade(permutations=1, nodes=bad)
    # fewer than 3 leaves in the other tree's subset
    cherry = next(int(v) for v in S.TreeA.get_internal_nodes() if len(S._leaves_below(S.TreeA, int(v))) == 2)
    S.subset_a(cherry)
    with pytest.raises(ValueError, match="at least 3 leaves"):
        S.hommola_by_clade(permutations=1)
    S.subset_a(S.TreeA.root_node)
    # ... and more than 16384
    big = _system(synth.balanced_tree(15), synth.balanced_tree(2), [(0, 0), (2, 2), (4, 4)])
    with pytest.raises(ValueError, match="at most 16384"):
        big.hommola_by_clade(permutations=1)
    mirror = big.hommola_by_clade(tree="A", permutations=1, max_leaves=16)      # (TreeB as the other tree: 4 leaves)
    assert mirror.n_leaves.tolist() == [16, 8, 4] and len(mirror.skipped_nodes) == 11
    # the C call's own checks reach Python as ValueError
    layout = ref.Layout(S.TreeB._flat.parent, S.TreeA._flat.parent, np.arange(32) * 2, np.arange(32) % 16 * 2)
    root = int(S.TreeB.root_node)
    dA, dB = S.TreeA._device_tree(), S.TreeB._device_tree()
    c = _clades(layout, [root])
    c["link_count"] -= 1
    with pytest.raises(ValueError, match="not the links inside"):
        dA.hommola_clades_host(dB, layout.univ_o, layout.univ_c, layout.pos_o, layout.pos_c, c, 1, 1)
    with pytest.raises(ValueError, match="non-decreasing"):
        dA.hommola_clades_host(dB, layout.univ_o, layout.univ_c, layout.pos_o, layout.pos_c[::-1].copy(), _clades(layout, [root]), 1, 1)
    with pytest.raises(_capi.InvalidNodeError):
        dA.hommola_clades_host(dB, layout.univ_o + S.TreeA.size, layout.univ_c, layout.pos_o, layout.pos_c, _clades(layout, [root]), 1, 1)
    empty = dA.hommola_clades_host(dB, layout.univ_o, layout.univ_c, layout.pos_o, layout.pos_c, _clades(layout, []), 3, 1)
    assert empty.shape == (0, 4)
