"""The topology test of phylosymbiosis on the host (CPU; device=None): SuchTree.dendrogram_congruence and
compare.dendrogram_congruence -- the observed match, the relabellings against match_clades calls with the ids permuted
by hand, the counts, the prefix property of the relabellings, min_branch over broken ties, and the argument errors."""
import numpy as np
import pytest

from linkage_reference import random_codes, ultrametric_codes
from suchtree_amd import SuchTree, _capi, compare

N = 64


@pytest.fixture(scope="module")
def ultrametric():
    """(the tree as a SuchTree -- never uploaded --, its leaf ids in object order, its own distances as codes)"""
    codes, _ = ultrametric_codes(N, 21)
    tree = compare.Dendrogram(N, "average", 0, _capi.linkage_codes(codes)).to_tree()
    assert isinstance(tree, SuchTree)
    return tree, np.array([tree.leaves[str(i)] for i in range(N)], dtype=np.int64), codes.astype(np.float64)


def test_a_tree_against_its_own_distances(ultrametric):
    tree, ids, y = ultrametric
    got = tree.dendrogram_congruence(y, ids, permutations=60, seed=5, keep_stats=True, device=None)
    assert isinstance(got, compare.TopologyTestResult)
    assert got.rf == 0 and got.rf_normalised == 0.0 and got.exact == got.n_a == got.n_b == N - 2 and got.transfer_total == 0 and got.mean_transfer == 0.0
    assert got.n_le == int((got.perm_rf == 0).sum()) and got.transfer_n_le == int((got.perm_transfer == 0).sum())
    assert got.p_value == (got.n_le + 1) / 61 and got.transfer_p_value == (got.transfer_n_le + 1) / 61
    assert got.perm_rf.dtype == np.int64 and got.perm_rf.shape == (60,) and (got.perm_rf > 0).any() and (got.perm_rf % 2 == 0).all()
    stat, p, n = got
    assert (stat, p, n) == (0, got.p_value, N)
    assert (got.linkage, got.rooted, got.permutations, got.seed, got.stream) == ("average", True, 60, 5, 0)
    assert got.leaves.tolist() == ids.tolist() and got.names == [str(i) for i in range(N)] and got.measure is None
    assert got.dendrogram.n == N and got.matches.rf == 0 and "rf=0" in repr(got)
    # leaf names do as well as ids, and the seed is drawn and reported when none is given
    again = tree.dendrogram_congruence(y, [str(i) for i in range(N)], permutations=60, seed=5, keep_stats=True, device=None)
    assert again.perm_rf.tolist() == got.perm_rf.tolist()
    assert tree.dendrogram_congruence(y, ids, permutations=1, device=None).seed is not None


@pytest.mark.parametrize("rooted", [True, False])
def test_relabellings_are_match_clades_with_the_ids_permuted(ultrametric, rooted):
    tree, ids, _ = ultrametric
    y = random_codes(N, 77).astype(np.float64)
    got = tree.dendrogram_congruence(y, ids, "complete", rooted=rooted, permutations=5, seed=9, stream=3, keep_stats=True, device=None)
    d_flat = got.dendrogram.to_flat()
    d_ids = np.array([d_flat.leaves[str(i)] for i in range(N)], dtype=np.int64)
    observed = compare.match_clades(d_flat, d_ids, tree._flat, ids, rooted=rooted, device=None)
    assert (got.rf, got.exact, got.n_a, got.n_b, got.transfer_total) == (observed.rf, observed.exact, observed.n_a, observed.n_b, int(observed.transfer.sum()))
    assert got.mean_transfer == observed.mean_transfer and got.matches.distance.tolist() == observed.distance.tolist()
    for p in range(1, 6):
        sigma = compare.hommola_permutation(9, 3, p, 0, N)
        by_hand = compare.match_clades(d_flat, d_ids[sigma], tree._flat, ids, rooted=rooted, device=None)      # object sigma[k] meets listed leaf k
        assert got.perm_rf[p - 1] == by_hand.rf and got.perm_transfer[p - 1] == int(by_hand.transfer.sum())
    assert got.n_le == int((got.perm_rf <= got.rf).sum()) and got.transfer_n_le == int((got.perm_transfer <= got.transfer_total).sum())


def test_the_first_relabellings_do_not_depend_on_how_many_are_asked_for(ultrametric):
    tree, ids, _ = ultrametric
    y = random_codes(N, 78).astype(np.float64)
    k = 7
    few = tree.dendrogram_congruence(y, ids, permutations=k, seed=2, keep_stats=True, device=None)
    many = tree.dendrogram_congruence(y, ids, permutations=3 * k, seed=2, keep_stats=True, device=None)
    assert few.perm_rf.tolist() == many.perm_rf[:k].tolist() and few.perm_transfer.tolist() == many.perm_transfer[:k].tolist()
    assert (few.rf, few.transfer_total) == (many.rf, many.transfer_total)
    assert many.n_le == int((many.perm_rf <= many.rf).sum()) and many.p_value == (many.n_le + 1) / (3 * k + 1)
    none = tree.dendrogram_congruence(y, ids, permutations=0, seed=2, keep_stats=True, device=None)
    assert none.p_value == 1.0 and len(none.perm_rf) == 0 and none.rf == few.rf
    assert tree.dendrogram_congruence(y, ids, permutations=k, seed=2, device=None).perm_rf is None
    # a Dendrogram is taken as it is
    given = tree.dendrogram_congruence(few.dendrogram, ids, permutations=k, seed=2, keep_stats=True, device=None)
    assert given.perm_rf.tolist() == few.perm_rf.tolist() and given.dendrogram is few.dendrogram


def test_min_branch_leaves_out_the_clades_of_broken_ties():
    # five points in three copies each: a triple merges at height 0 twice, and the first of the two clades has a branch of 0
    rng = np.random.default_rng(4)
    points = np.repeat(rng.random((5, 3)), 3, axis=0)
    n = len(points)
    y = np.sqrt(((points[:, None, :] - points[None, :, :]) ** 2).sum(axis=2))
    tree = compare.linkage(random_codes(n, 5).astype(np.float64), device=None).to_tree()
    ids = np.array([tree.leaves[str(i)] for i in range(n)], dtype=np.int64)
    every = tree.dendrogram_congruence(y, ids, permutations=9, seed=1, device=None)
    kept = tree.dendrogram_congruence(y, ids, min_branch=0.0, permutations=9, seed=1, device=None)
    assert every.n_a == n - 2 and kept.n_a == n - 2 - 5 and kept.n_b == every.n_b == n - 2
    assert (every.dendrogram.heights[:10] == 0.0).all() and every.dendrogram.heights[10] > 0.0
    sizes = sorted(kept.matches.n_leaves.tolist())
    assert sizes.count(3) == 5 and sizes.count(2) == 0


def test_argument_errors(ultrametric):
    tree, ids, y = ultrametric
    with pytest.raises(ValueError, match="linkage must be one of"):
        tree.dendrogram_congruence(y, ids, "ward", device=None)
    with pytest.raises(ValueError, match="a repeated leaf"):
        tree.dendrogram_congruence(y, np.r_[ids[:-1], ids[0]], device=None)
    with pytest.raises(ValueError, match="3 leaves: 4 to 16384"):
        tree.dendrogram_congruence(y[:3], ids[:3], device=None)
    with pytest.raises(ValueError, match="y is over 5 objects, not over the 64 leaves"):
        tree.dendrogram_congruence(y[:10], ids, device=None)
    for kw in ({"permutations": -1}, {"seed": -1}, {"stream": -1}):
        with pytest.raises(ValueError):
            tree.dendrogram_congruence(y, ids, device=None, **kw)
    with pytest.raises(ValueError, match="is not a leaf"):
        tree.dendrogram_congruence(y, np.r_[ids[:-1], tree.root_node], device=None)
