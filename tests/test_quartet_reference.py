"""tests/quartet_reference.py against brute force, before tests/test_gpu_quartet_edges.py trusts it (no GPU)."""
import itertools
import math

import numpy as np
import pytest

import quartet_reference as qr
from oracle.oracle import OracleTree
from suchtree_amd import synth
from suchtree_amd.compare import quartet_positions


# ---- which quartet is quartet k -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(0, 13))
def test_colex_quartets_against_sorted_combinations(m):
    want = sorted(itertools.combinations(range(m), 4), key=lambda t: t[::-1])
    got = qr.colex_quartets(m)
    assert got.shape == (math.comb(m, 4), 4) and got.tolist() == [list(t) for t in want]


def test_colex_quartets_against_a_lexsort_of_the_reversed_columns():
    c = np.array(list(itertools.combinations(range(30), 4)), dtype=np.int64)
    want = c[np.lexsort((c[:, 0], c[:, 1], c[:, 2], c[:, 3]))]      # (the last key is the primary one)
    assert np.array_equal(qr.colex_quartets(30), want)


def test_unrank_exact_against_colex_quartets():
    want = qr.colex_quartets(30)
    assert [qr.unrank_exact(k) for k in range(len(want))] == want.tolist()
    # where a floating-point root is of no use: the last quartet of 65536 leaves and the block edge before it
    total = math.comb(65536, 4)
    assert qr.unrank_exact(total - 1) == [65532, 65533, 65534, 65535]
    assert qr.unrank_exact(math.comb(65535, 4)) == [0, 1, 2, 65535]
    assert qr.unrank_exact(math.comb(65535, 4) - 1) == [65531, 65532, 65533, 65534]


def test_the_host_restatement_against_colex_quartets_at_103_leaves():
    got = quartet_positions(103)
    assert len(got) == 4_421_275 == (1 << 22) + 226_971 and np.array_equal(got, qr.colex_quartets(103))


def test_py_draw_gives_four_distinct_positions_and_every_order():
    rows = [qr.py_draw(7, k, 5) for k in range(3000)]
    assert all(len(set(r)) == 4 and min(r) >= 0 and max(r) < 5 for r in rows) and len({tuple(r) for r in rows}) == 120
    assert sorted(qr.py_draw((1 << 64) - 1, (1 << 62) - 1, 4)) == [0, 1, 2, 3]


# ---- the class of a quartet -----------------------------------------------------------------------------------------
def oracle_classes(O, quartets):
    """Class of each row (distinct ids) from OracleTree.quartets: which input column ends up beside column 0."""
    q = np.ascontiguousarray(quartets, dtype=np.int64)
    out = O.quartets(q)
    at = np.argmax(out == q[:, :1], axis=1)                 # where column 0 went
    partner = out[np.arange(len(q)), at ^ 1]                # its sister
    cls = np.argmax(q[:, 1:] == partner[:, None], axis=1)   # input column 1, 2 or 3 -> class 0, 1, 2
    assert (out[np.arange(len(q)), at] == q[:, 0]).all() and (q[np.arange(len(q)), cls + 1] == partner).all()
    return cls


def pick_classes(m6):
    """The pick rule over (n, 6) MRCA ids in the order ab ac ad bc bd cd: the first id that occurs once decides."""
    counts = (m6[:, :, None] == m6[:, None, :]).sum(axis=2)
    unique = counts == 1
    pick = np.where(unique.any(axis=1), np.argmax(unique, axis=1), 6)
    return np.where(pick == 6, 3, np.where(pick < 3, pick, 5 - pick))


def mrca_ids(M, pos):
    return np.stack([M[pos[:, i], pos[:, j]] for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))], axis=1)


def shuffled_quartets(m, n, seed):
    """n rows of four distinct positions below m, in every order of the four."""
    rng = np.random.default_rng(seed)
    return np.argsort(rng.random((n, m)), axis=1)[:, :4]


@pytest.mark.parametrize("name", ["random", "balanced", "caterpillar"])
def test_leaf_classes_on_binary_trees_against_the_pick_rule_and_the_oracle(name):
    parent, dist = {"random": lambda: synth.random_binary_tree(200, seed=5), "balanced": lambda: synth.balanced_tree(6),
                    "caterpillar": lambda: synth.caterpillar_tree(40)}[name]()
    ids = np.random.default_rng(8).permutation(np.arange((len(parent) + 1) // 2, dtype=np.int64) * 2)
    D, M = qr.mrca_matrices(parent, ids)
    pos = np.concatenate([shuffled_quartets(len(ids), 20_000, 9), qr.colex_quartets(min(len(ids), 25))])
    got = qr.leaf_classes(parent, ids, pos, D=D)
    assert np.array_equal(got, qr.leaf_classes(parent, ids, pos))
    assert got.max() <= 2 and set(got.tolist()) == {0, 1, 2}
    assert np.array_equal(got, pick_classes(mrca_ids(M, pos)))
    assert np.array_equal(got, oracle_classes(OracleTree(parent, dist), ids[pos]))
    # the MRCA ids themselves, against the oracle's
    i, j = np.triu_indices(len(ids), 1)
    assert np.array_equal(M[i, j], OracleTree(parent, dist).mrca_bulk(np.stack([ids[i], ids[j]], axis=1)))


@pytest.mark.parametrize("parent, want", [
    ([-1, 0, 0, 0, 0], 3),               # (a,b,c,d)
    ([5, 5, 5, 4, -1, 4], 3),            # ((a,b,c),d): nodes a b c d root x
    ([5, 5, 4, 4, -1, 4], 0),            # ((a,b),c,d)
    ([4, 4, 5, 5, -1, 4], 0),            # (a,b,(c,d))
])
def test_leaf_classes_on_hand_written_polytomies(parent, want):
    ids = np.arange(1, 5) if len(parent) == 5 else np.arange(4)
    assert qr.leaf_classes(parent, ids, [[0, 1, 2, 3]]).tolist() == [want]
    # the same four leaves in the other column orders: the sisters' columns decide the class
    if want == 0:
        assert qr.leaf_classes(parent, ids, [[0, 2, 1, 3], [0, 2, 3, 1], [2, 3, 0, 1], [3, 1, 0, 2]]).tolist() == [1, 2, 0, 2]
    else:
        assert qr.leaf_classes(parent, ids, [[0, 2, 1, 3], [3, 2, 1, 0]]).tolist() == [3, 3]


def test_the_closed_forms_against_leaf_classes():
    v = [0, 1, 2, 3, 4, 7, 8, 127, 128, 2 ** 31 - 1, 2 ** 31, 2 ** 53 - 1]
    assert qr._bit_length(np.array(v, dtype=np.int64)).tolist() == [x.bit_length() for x in v]
    parent, _, ids = qr.perfect_tree(6)
    perm = np.random.default_rng(6).permutation(64)
    pos = qr.colex_quartets(64)
    assert np.array_equal(qr.perfect_classes(6, pos), qr.leaf_classes(parent, ids, pos))
    got = qr.perfect_classes(6, perm[pos])
    assert np.array_equal(got, qr.leaf_classes(parent, ids[perm], pos)) and set(got.tolist()) == {0, 1, 2}
    pos = qr.colex_quartets(40)
    parent, _, ids = qr.caterpillar(40)
    assert np.array_equal(qr.caterpillar_classes(pos), qr.leaf_classes(parent, ids, pos))
    assert np.array_equal(qr.caterpillar_classes(pos), qr.leaf_classes(parent, ids[::-1], pos))      # deepest first
    cp, _ = synth.caterpillar_tree(40)
    assert np.array_equal(qr.caterpillar_classes(pos), qr.leaf_classes(cp, np.arange(40) * 2, pos))
    parent, _, ids = qr.star(40)
    assert np.array_equal(qr.star_classes(pos), qr.leaf_classes(parent, ids, pos))


# ---- trees ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_leaves, seed", [(2, 0), (5, 1), (300, 2), (300, 3)])
def test_random_general_tree_is_a_tree_of_the_stated_shape(n_leaves, seed):
    parent, dist, leaves = qr.random_general_tree(n_leaves, seed)
    n = len(parent)
    children = np.bincount(parent[parent >= 0], minlength=n)
    assert (parent < 0).sum() == 1 and dist[parent < 0] == -1.0 and (dist[parent >= 0] > 0).all()
    assert sorted(leaves.tolist()) == np.flatnonzero(children == 0).tolist() and len(leaves) == n_leaves
    assert set(children[children > 0].tolist()) <= {2, 3, 4, 5} and (qr.node_depths(parent) >= 0).all()
    if n_leaves == 300:
        assert {2, 3, 4, 5} == set(children[children > 0].tolist())
        assert (leaves % 2).any() and (np.diff(leaves) < 0).any()      # neither the even ids nor in order


def test_table_of_counts_the_pairs():
    t = qr.table_of([0, 0, 3, 2, 0], [1, 1, 3, 0, 2])
    assert t.sum() == 5 and t[0, 1] == 2 and t[3, 3] == 1 and t[2, 0] == 1 and t[0, 2] == 1
