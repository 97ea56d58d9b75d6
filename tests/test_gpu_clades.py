"""Every clade at once on the GPU (SuchLinkedTrees.linked_distances_by_clade, C ABI st_compare_clades_host): every row
against subset_x(node); linked_distances() reduced with numpy float64."""
import numpy as np
import pandas as pd
import pytest
from scipy.stats import beta, pearsonr

from conftest import golden_path
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_moments(c, x, y):      # (the bars of tests/test_gpu_compare.py)
    assert c.n_pairs == len(x)
    for got, want in ((c.mean_x, x.mean()), (c.mean_y, y.mean()), (c.var_x, np.var(x)), (c.var_y, np.var(y)),
                      (c.cov, np.cov(x, y, bias=True)[0, 1])):
        assert _rel(got, want) < 1e-10, (got, want)
    dx, dy = x - c.shift_x, y - c.shift_y
    for got, want in ((c.sxx, (dx * dx).sum()), (c.syy, (dy * dy).sum()), (c.sxy, (dx * dy).sum())):
        assert _rel(got, want) < 1e-10 or abs(got - want) < 1e-12, (got, want)
    assert abs(c.sx - dx.sum()) <= 1e-10 * np.sqrt(len(x) * c.sxx) and abs(c.sy - dy.sum()) <= 1e-10 * np.sqrt(len(y) * c.syy)
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max())


def _check_row(S, C, i, node, tree):
    """Row i of C against the loop of the notebook for clade ``node``."""
    if tree == "B":
        S.subset_b(int(node))
        n_leaves = S.subset_b_size
    else:
        S.subset_a(int(node))
        n_leaves = S.subset_a_size
    res = S.linked_distances()
    x, y = res["TreeA"], res["TreeB"]
    assert C.n_links[i] == S.subset_n_links and C.n_leaves[i] == n_leaves and C.n_pairs[i] == len(x)
    c = C.comparison(node)
    assert c.n_leaves == S.subset_n_links
    _check_moments(c, x, y)
    if np.var(x) == 0 or np.var(y) == 0:
        assert np.isnan(C.pearson_r[i])
    else:
        r, p = pearsonr(x, y)
        assert abs(C.pearson_r[i] - r) < 1e-12
        # p's relative sensitivity to r is about n |r| / (1 - r^2): r's last bits (1e-13 here) move a p of 1e-22 by 3e-5
        # relative.  So: 1e-9 of pearsonr's own p-value function at this r, and pearsonr's p to what r's error allows
        n = len(x)
        at_r = 2 * beta(n / 2 - 1, n / 2 - 1, loc=-1, scale=2).sf(abs(C.pearson_r[i]))
        assert abs(C.pvalue[i] - at_r) <= 1e-9 * at_r + 1e-300, (C.pvalue[i], at_r)
        if abs(r) < 1 - 1e-6:      # (at |r| = 1 in the last bits p jumps to 0: scipy clips r)
            slack = n * abs(r) / (1 - r * r) * (abs(C.pearson_r[i] - r) + 1e-15)
            assert abs(C.pvalue[i] - p) <= (1e-9 + 4 * slack) * p + 1e-300, (C.pvalue[i], p)


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


def _state(S):
    return (S.subset_a_root, S.subset_b_root, S.subset_a_size, S.subset_b_size, S.subset_n_links,
            S.subset_a_leafs.copy(), S.subset_b_leafs.copy(), S.linklist.copy())


def _same_state(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("tree", ["B", "A"])
@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
def test_fixtures_every_clade(which, tree):
    S = _slt(which)
    before = _state(S)
    C = S.linked_distances_by_clade(tree=tree)
    assert _same_state(before, _state(S))
    clade_tree = S.TreeB if tree == "B" else S.TreeA
    internal = clade_tree.get_internal_nodes()
    # every internal node with at least two links has a row, in get_internal_nodes() order
    assert np.array_equal(C.nodes, [v for v in internal if v in set(C.nodes.tolist())])
    assert len(C) > 3
    R = _slt(which)
    for i, node in enumerate(C.nodes):
        _check_row(R, C, i, node, tree)
    df = C.to_dataframe()
    assert len(df) == len(C) and df["name"][0] == "clade_%d" % C.nodes[0]


@pytest.fixture(scope="module")
def synthetic():
    pa, da = synth.balanced_tree(8)
    pb, db = synth.random_binary_tree(5000, seed=3)
    A = SuchTree((pa, da, ["a%d" % i for i in range(256)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(5000)]))
    rows = np.random.default_rng(8).integers(0, 256, 5000)
    mat = np.zeros((256, 5000), dtype=np.int64)
    mat[rows, np.arange(5000)] = 1
    return A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves))


@pytest.mark.parametrize("step", ["whole", "subset_a"])
def test_synthetic_root_and_300_clades_and_cap(synthetic, step):
    A, B, df = synthetic
    S = SuchLinkedTrees(A, B, df)
    R = SuchLinkedTrees(A, B, df)
    if step == "subset_a":
        S.subset_a(int(A.get_children(A.root_node)[0]))
        R.subset_a(int(A.get_children(A.root_node)[0]))
    before = _state(S)
    C = S.linked_distances_by_clade()
    assert _same_state(before, _state(S))
    assert C.nodes[0] == B.root_node
    rng = np.random.default_rng(11)
    pick = [0] + sorted(rng.choice(np.arange(1, len(C)), size=300, replace=False).tolist())
    for i in pick:
        _check_row(R, C, i, C.nodes[i], "B")
    # a cap: the same bits for every row within it, no row above it
    cap = 40
    K = S.linked_distances_by_clade(max_links=cap)
    assert len(K) and K.n_links.max() <= cap
    within = C.nodes[C.n_links <= cap]
    assert np.array_equal(K.nodes, within)
    row = {int(v): i for i, v in enumerate(C.nodes)}
    sel = np.array([row[int(v)] for v in K.nodes])
    for col in ("n_pairs", "shift_x", "shift_y", "sx", "sy", "sxx", "syy", "sxy", "min_a", "max_a", "min_b", "max_b", "pearson_r"):
        assert np.array_equal(getattr(K, col), getattr(C, col)[sel], equal_nan=True), col


def test_deterministic_across_calls_and_chunk_sizes(synthetic):
    A, B, df = synthetic
    S = SuchLinkedTrees(A, B, df)
    C1 = S.linked_distances_by_clade()
    C2 = S.linked_distances_by_clade()
    C3 = S.linked_distances_by_clade(chunk_pairs=_capi.CLADE_TILE)
    for col in ("n_pairs", "shift_x", "shift_y", "sx", "sy", "sxx", "syy", "sxy", "min_a", "max_a", "min_b", "max_b"):
        a, b, c = getattr(C1, col), getattr(C2, col), getattr(C3, col)
        assert a.tobytes() == b.tobytes() == c.tobytes(), col
    with pytest.raises(ValueError):
        S.linked_distances_by_clade(chunk_pairs=_capi.CLADE_TILE + 1)


def test_deep_caterpillar_clade_tree():
    pa, da = synth.balanced_tree(6)
    pb, db = synth.caterpillar_tree(3000)
    A = SuchTree((pa, da, ["a%d" % i for i in range(64)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(3000)]))
    rng = np.random.default_rng(4)
    mat = np.zeros((64, 3000), dtype=np.int64)
    mat[rng.integers(0, 64, 3000), np.arange(3000)] = 1
    mat[rng.integers(0, 64, 3000), np.arange(3000)] = 1      # one or two links per TreeB leaf
    S = SuchLinkedTrees(A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves)))
    C = S.linked_distances_by_clade(min_leaves=10)
    assert len(C) == 3000 - 1 - 8      # internal nodes with >= 10 leaves
    R = SuchLinkedTrees(A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves)))
    for i in [0, 1, 2, 500, 1700, len(C) - 1]:
        _check_row(R, C, i, C.nodes[i], "B")


def test_argument_errors_on_the_gpu(synthetic):
    A, B, df = synthetic
    dA, dB = A._device_tree(), B._device_tree()
    parent = B._flat.parent
    leaf_b = np.asarray(B.leaf_node_ids[:4], dtype=np.int64)
    with pytest.raises(ValueError):          # a parent array of the wrong size
        dA.compare_clades_host(dB, parent[:-1], np.array([0, 1, 2, 3]), leaf_b)
    with pytest.raises(ValueError):          # a link that is not a leaf of the clade tree
        dA.compare_clades_host(dB, parent, np.array([0, 1]), np.array([leaf_b[0], B.root_node]))
    with pytest.raises(_capi.InvalidNodeError):
        dA.compare_clades_host(dB, parent, np.array([0, A.size + 9]), leaf_b[:2])
    with pytest.raises(_capi.InvalidNodeError):
        dA.compare_clades_host(dB, parent, np.array([0, 1]), np.array([leaf_b[0], B.size + 2]))
    if _capi.device_count() < 2:
        return
    other = SuchTree((B._flat.parent, B._flat.distance), device=1)
    with pytest.raises(ValueError):
        dA.compare_clades_host(other._device_tree(), parent, np.array([0, 1]), leaf_b[:2])
