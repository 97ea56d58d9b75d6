"""k_rf_tasks on the GPU: st_rf_tasks(device = 0) against its host restatement (device = -1), integer for integer on the
shared counts and on the per-clade counts, and against the set oracle of rf_reference.py where m <= 129: the edges of the
blocks of 64 positions, several blocks and table levels (an odd block count across a level), the cap with the whole LDS
budget, more tasks than the grid and than a chunk, triangle ranges that split a row, explicit tasks with alignments, empty
clade lists, and the two facades against transfer_support and dendrogram_congruence.  Every comparison is exact."""
import numpy as np
import pytest

import rf_reference as ref
from clade_match_reference import random_tree, shuffled_tree
from suchtree_amd import SuchTree, _capi, compare, synth

pytestmark = pytest.mark.gpu


def _both(m, sides, rooted, what, **kw):
    """(shared, counts) of the kernel, checked against the restatement's"""
    where, offsets, lo, hi = sides[:4]
    host_kw = {k: v for k, v in kw.items() if k != "chunk_tasks"}
    want = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, device=-1, **host_kw)
    got = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, device=0, **kw)
    for name, g, w in zip(("shared", "counts"), got, want):
        if w is None:
            assert g is None
            continue
        bad = np.flatnonzero(g != w)
        assert g.dtype == w.dtype and len(bad) == 0, "%s: %d of %d %s differ, first at %d: got %d want %d" % (what, len(bad), len(w), name, bad[0], g[bad[0]],
                                                                                                              w[bad[0]])
    return got


def _complement_tasks(where, offsets, lo, hi):
    """the tasks (i, j) of the triangle in which a clade of j holds the leaf at i's position 0"""
    out = []
    for i, j in ref.triangle(len(where)):
        noted = where[j][np.flatnonzero(where[i] == 0)[0]]
        l, h = lo[offsets[j]:offsets[j + 1]], hi[offsets[j]:offsets[j + 1]]
        if ((l <= noted) & (noted < h)).any():
            out.append((i, j))
    return out


@pytest.mark.parametrize("rooted", [False, True])
@pytest.mark.parametrize("m", [4, 5, 63, 64, 65, 128, 129])
def test_block_edges_against_restatement_and_sets(m, rooted):
    trees = ref.tree_set(m, 1000 + m)
    sets = [ref.clade_sets(parent, ids, rooted) for parent, ids in trees]
    sides = ref.library_sides(trees, rooted)
    shared, counts = _both(m, sides, rooted, "m %d rooted %s" % (m, rooted))
    pairs = ref.triangle(len(trees))
    assert shared.tolist() == [ref.shared(sets[i], sets[j]) for i, j in pairs]
    freq = ref.frequencies(sets)
    assert counts.tolist() == [freq[s] - 1 for side in sides[4] for s in ref.side_sets(side, rooted)]
    if not rooted and m > 4:
        assert _complement_tasks(*sides[:4])      # (the complement path is taken)
        # the root's two children are one bipartition: the random tree lists m - 3 clades, not m - 2
        assert sides[1][1] - sides[1][0] == m - 3 and shared[0] == m - 3
    # alignments, against the sets
    rng = np.random.default_rng(m)
    align = np.stack([np.arange(m)] + [rng.permutation(m) for _ in range(3)]).astype(np.int32)
    ti, tj, tp = (rng.integers(0, top, size=40).astype(np.int32) for top in (len(trees), len(trees), 4))
    got, _ = _both(m, sides, rooted, "aligned, m %d" % m, align=align, task_i=ti, task_j=tj, task_p=tp)
    assert got.tolist() == [ref.shared(sets[i], sets[j], align[p], rooted) for i, j, p in zip(ti, tj, tp)]


def _levels_trees(m, seed, n=3):
    leaves = np.arange(m, dtype=np.int64) * 2
    return [(synth.random_binary_tree_levels(m, seed=seed + t)[0], leaves[np.random.default_rng(seed + 10 + t).permutation(m)] if t else leaves)
            for t in range(n)]


@pytest.mark.parametrize("m", [4097, 8193])
def test_several_blocks_and_table_levels(m):
    trees = _levels_trees(m, 3 * m)
    trees[2] = (trees[0][0], trees[0][1][::-1].copy())      # (tree 0's shape with the leaves dealt backwards: a few clades are shared)
    for rooted in (False, True):
        sides = ref.library_sides(trees, rooted)
        shared, _ = _both(m, sides, rooted, "m %d rooted %s" % (m, rooted))
        assert 0 <= shared[0] < sides[1][1]
        rng = np.random.default_rng(m)
        align = np.stack([rng.permutation(m) for _ in range(4)] + [np.arange(m)]).astype(np.int32)
        ti, tj, tp = np.array([0, 1, 2, 0, 2, 1, 0], dtype=np.int32), np.array([1, 2, 0, 0, 2, 0, 0], dtype=np.int32), np.array([0, 1, 2, 3, -1, 4, 4], dtype=np.int32)
        got, _ = _both(m, sides, rooted, "aligned, m %d" % m, align=align, task_i=ti, task_j=tj, task_p=tp)
        assert got[4] == sides[1][3] - sides[1][2] and got[6] == sides[1][1] and got[5] == shared[0]


def test_the_cap_and_the_whole_lds_budget():
    m = _capi.RF_MAX_LEAVES
    cat = synth.caterpillar_tree(m)[0]
    ids = (np.random.default_rng(1).permutation(m) * 2).astype(np.int64)
    trees = [(cat, ids), (np.asarray(synth.complete_tree(m)[0], dtype=np.int32), (np.random.default_rng(2).permutation(m) * 2).astype(np.int64)),
             (cat.copy(), ids.copy())]
    for rooted in (False, True):
        sides = ref.library_sides(trees, rooted)
        where, offsets, lo, hi, per_tree = sides
        shared, counts = _both(m, sides, rooted, "cap, rooted %s" % rooted)
        n_cat = m - 2 if rooted else m - 3
        assert np.diff(offsets).tolist() == [n_cat, m - 2 if rooted else m - 3, n_cat]
        assert shared[1] == n_cat and (counts[:n_cat] >= 1).all()      # (the identical pair)
        assert sorted(set((hi - lo)[:n_cat].tolist())) == list(range(2, n_cat + 2))      # (ranges of every size)
        # the third witness: the delta-0 rows of st_clade_match on the device, caterpillar against balanced
        i, j = 1, 0
        pos_b = where[j][per_tree[i][0]]
        distance, match, _ = _capi.clade_match(m, pos_b, per_tree[i][2], per_tree[i][3], per_tree[j][2], per_tree[j][3], rooted, 0)
        assert int(((match >= 0) & (distance == 0)).sum()) == shared[0]


def _small_trees(n_trees, m):
    """n_trees trees of m leaves: twenty shapes, the leaves dealt in an order a few transpositions away from the first"""
    out = []
    for t in range(n_trees):
        order = np.arange(m)
        rng = np.random.default_rng(500 + t)
        for _ in range(t // 20):
            a, b = rng.integers(0, m, size=2)
            order[[a, b]] = order[[b, a]]
        out.append((synth.random_binary_tree(m, seed=t % 20)[0], (order * 2).astype(np.int64)))
    return out


def test_more_tasks_than_the_grid_and_than_a_chunk():
    m, n = 33, 200
    trees = _small_trees(n, m)
    total = n * (n - 1) // 2
    for rooted in (False, True):
        sides = ref.library_sides(trees, rooted)
        where, offsets, lo, hi = sides[:4]
        shared, counts = _both(m, sides, rooted, "200 trees, rooted %s" % rooted)
        assert len(shared) == total == 19900 and len(set(shared.tolist())) > 3 and shared.max() <= m - (2 if rooted else 3)
        for chunk in (1, 7):
            got = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, device=0, chunk_tasks=chunk)
            assert (got[0] == shared).all() and (got[1] == counts).all(), chunk
        # ranges that split a row: row 100 is pairs [4950, 5050)
        cuts = [0, 4990, 5001, 19000, total]
        parts = [_capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, begin=b, count=e - b, want_count=False, device=0, chunk_tasks=c)[0]
                 for b, e, c in zip(cuts, cuts[1:], (0, 1, 4097, 7))]
        assert (np.concatenate(parts) == shared).all()


def test_explicit_tasks_with_alignments():
    m = 200
    # (the leaves of an in-order tree are its even ids) tree 2 is tree 0 with the common leaves dealt in another order
    trees = [(synth.random_binary_tree(m, seed=1)[0], np.arange(m, dtype=np.int64) * 2), (synth.random_binary_tree(m, seed=2)[0], np.arange(m, dtype=np.int64) * 2),
             (synth.random_binary_tree(m, seed=1)[0], (np.random.default_rng(4).permutation(m) * 2).astype(np.int64))]
    rng = np.random.default_rng(5)
    align = np.stack([rng.permutation(m) for _ in range(64)]).astype(np.int32)
    align[17] = np.arange(m)
    # row 40 undoes the dealing of tree 2: under it tree 2 is tree 0
    align[40] = np.argsort(trees[2][1])
    ti, tj, tp = (rng.integers(0, top, size=300).astype(np.int32) for top in (3, 3, 64))
    tp[rng.random(300) < 0.2] = -1
    ti[:6], tj[:6], tp[:6] = [0, 1, 2, 0, 0, 2], [0, 1, 2, 2, 2, 0], [-1, 17, -1, 40, 17, -1]
    for rooted in (False, True):
        sides = ref.library_sides(trees, rooted)
        n0 = sides[1][1]
        for want_count in (True, False):
            got, counts = _both(m, sides, rooted, "explicit, rooted %s" % rooted, align=align, task_i=ti, task_j=tj, task_p=tp, want_count=want_count,
                                chunk_tasks=64)
            assert (counts is None) == (not want_count)
            assert got[:3].tolist() == np.diff(sides[1]).tolist() and got[4] == got[5] < n0 and got[3] == n0
        named = _both(m, sides, rooted, "identity row", align=align, task_i=ti, task_j=tj, task_p=np.full(300, 17, dtype=np.int32))[0]
        plain = _both(m, sides, rooted, "identity", task_i=ti, task_j=tj)[0]
        assert (named == plain).all()


def test_a_star_and_a_list_that_min_branch_emptied():
    m = 70
    names = ["L%d" % k for k in range(m)]
    a, b = random_tree(m, 21), shuffled_tree(m, 22, 23)
    parent, distance = synth.random_binary_tree(m, seed=24, zero_fraction=1.0)      # (every branch is the polytomy epsilon)
    flat = SuchTree((parent, distance, names))
    for rooted in (False, True):
        with_it = compare.tree_set([a, flat, b, a], rooted=rooted, min_branch=1e-9, device=0)
        host = compare.tree_set([a, flat, b, a], rooted=rooted, min_branch=1e-9, device=None)
        without = compare.tree_set([a, b, a], rooted=rooted, min_branch=1e-9, device=0)
        assert with_it.n_clades.tolist() == [without.n_clades[0], 0, without.n_clades[1], without.n_clades[2]] and with_it.n_clades[0] > 0
        assert with_it.shared.tolist() == host.shared.tolist() and with_it.shared[[0, 2, 4]].tolist() == [0, 0, 0]
        assert with_it.shared[[1, 3, 5]].tolist() == without.shared.tolist() and with_it.shared[3] == with_it.n_clades[0]
        for t, s in ((0, 0), (2, 1), (3, 2)):
            assert with_it.clades(t)[2].tolist() == without.clades(s)[2].tolist() == host.clades(t)[2].tolist()
        assert len(with_it.clades(1)[2]) == 0
        # the same at the call itself: tree 1 of three is a star
        trees = ref.tree_set(m, 9)
        sides = ref.library_sides([trees[0], trees[5], trees[6]], rooted)
        shared, counts = _both(m, sides, rooted, "star")
        assert sides[1].tolist()[1] == sides[1].tolist()[2] and shared[0] == shared[2] == 0


def test_tree_set_on_newick_replicates():
    a = random_tree(500, 14)
    newick = lambda t: synth.to_newick(t._flat.parent, t._flat.distance, t.leaf_nodes)      # noqa: E731
    reps = [newick(shuffled_tree(500, 15 + 2 * k, 16 + 2 * k)) for k in range(8)] + [newick(a)] + [newick(shuffled_tree(500, 14, 40 + k)) for k in range(3)]
    assert len(reps) == 12
    for rooted in (False, True):
        dev = compare.tree_set([a] + reps, rooted=rooted, device=0)
        host = compare.tree_set([a] + reps, rooted=rooted, device=None)
        default = compare.tree_set([a] + reps, rooted=rooted)
        for other in (host, default):
            assert dev.count == other.count == 78 and dev.n_clades.tolist() == other.n_clades.tolist()
            for k in ("shared", "rf", "i", "j"):
                assert getattr(dev, k).dtype == np.int64 and getattr(dev, k).tolist() == getattr(other, k).tolist(), k
            assert dev.rf_normalised.tobytes() == other.rf_normalised.tobytes()
            for t in range(13):
                for x, y in zip(dev.clades(t), other.clades(t)):
                    assert x.tolist() == y.tolist()
        support = a.transfer_support(reps, rooted=rooted)
        nodes, n_leaves, frequency = dev.clades(0)
        assert nodes.tolist() == support.nodes.tolist() and (frequency - 1).tolist() == support.exact_count.tolist() and (frequency >= 2).all()
        assert dev.pair(36) == (9, 0) and dev.shared[36] == dev.n_clades[0] and dev.matrix("rf")[9, 0] == 0


@pytest.mark.parametrize("rooted", [True, False])
def test_rf_relabelled_is_the_rf_column_of_dendrogram_congruence(rooted):
    from linkage_reference import random_codes
    n = 300
    tree = compare.linkage(random_codes(n, 5).astype(np.float64), device=None).to_tree()
    ids = np.array([tree.leaves[str(i)] for i in range(n)], dtype=np.int64)
    y = random_codes(n, 6).astype(np.float64)
    want = compare.dendrogram_congruence(tree._flat, ids, y, rooted=rooted, permutations=99, seed=13, keep_stats=True, device=0)
    d_flat = want.dendrogram.to_flat()
    d_ids = np.array([d_flat.leaves[str(i)] for i in range(n)], dtype=np.int64)
    got = compare.rf_relabelled(tree._flat, ids, d_flat, d_ids, permutations=99, seed=13, rooted=rooted, device=0)
    host = compare.rf_relabelled(tree._flat, ids, d_flat, d_ids, permutations=99, seed=13, rooted=rooted, device=None)
    assert got.perm_rf.tolist() == want.perm_rf.tolist() == host.perm_rf.tolist()
    assert (got.rf, got.n_le, got.p_value) == (want.rf, want.n_le, want.p_value) == (host.rf, host.n_le, host.p_value)
    assert got.shared == want.exact and (got.n_a, got.n_b) == (want.n_b, want.n_a)


def test_arguments_are_checked_before_the_device():
    where = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], dtype=np.int32)
    with pytest.raises(ValueError, match=r"where\[1\]\[4\] = 3"):
        _capi.rf_tasks(5, np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 3]]), [0, 0, 0], [], [], device=0)
    with pytest.raises(IndexError, match="task 0: trees"):
        _capi.rf_tasks(5, where, [0, 0, 0], [], [], task_i=[2], task_j=[0], device=0)
    with pytest.raises(ValueError, match="device"):
        _capi.rf_tasks(5, where, [0, 0, 0], [], [], device=_capi.device_count())
    shared, counts = _capi.rf_tasks(5, where, [0, 0, 0], [], [], device=0)      # (two stars)
    assert shared.tolist() == [0] and counts.tolist() == []
