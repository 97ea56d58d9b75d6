"""k_clade_match on the GPU: st_clade_match(device = 0) against its host restatement (device = -1), integer for integer
on all three outputs, and against the brute-force set reference where m <= 129: the word edges of the LDS bitmap (rank(m)
at a multiple of 64 included), scans of several words per thread, the cap with the whole LDS budget, more rows than a
chunk and than the grid, both modes, a near-complement, identical trees, balanced against caterpillar, a tie, no
candidates, the size windows on and off, and the two facade calls.  Every comparison is exact."""
import numpy as np
import pytest

import clade_match_reference as ref
from conftest import golden_path
from suchtree_amd import SuchTree, _capi, synth

pytestmark = pytest.mark.gpu

WINDOW = "SUCHTREE_AMD_CLADE_MATCH_WINDOW"


def _same(got, want, what):
    for name, g, w in zip(("distance", "match", "intersection"), got, want):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s: %d of %d %s differ, first at row %d: got %d want %d" % (what, len(bad), len(w), name, bad[0], g[bad[0]], w[bad[0]])


def _both(args, rooted, what, **kw):
    """The kernel's outputs, checked against the restatement's."""
    want = _capi.clade_match(*args, rooted=rooted, device=-1)
    got = _capi.clade_match(*args, rooted=rooted, device=0, **kw)
    _same(got, want, what)
    return got


def _levels_case(m, seed):
    """(m, pos_b, a_lo, a_hi, b_lo, b_hi) per mode of two seeded random trees of m leaves whose leaf lists are shuffled
    against one another: the library's range builder on parent arrays, no tree object."""
    pa, _ = synth.random_binary_tree_levels(m, seed=seed)
    pb, _ = synth.random_binary_tree_levels(m, seed=seed + 1)
    leaves = np.arange(m, dtype=np.int64) * 2      # (in-order ids: the leaves are the even ones)
    ids_b = leaves[np.random.default_rng(seed + 2).permutation(m)]
    out = {}
    for rooted in (False, True):
        side_a, side_b = _capi.clade_ranges(pa, leaves, rooted), _capi.clade_ranges(pb, ids_b, rooted)
        where_b = np.empty(m, dtype=np.int32)
        where_b[side_b[0]] = np.arange(m, dtype=np.int32)
        out[rooted] = (m, where_b[side_a[0]], side_a[2], side_a[3], side_b[2], side_b[3])
    return out


@pytest.mark.parametrize("m", [4, 5, 63, 64, 65, 128, 129])
def test_word_edges_against_restatement_and_sets(m):
    a, b = ref.random_tree(m, 100 + m), ref.shuffled_tree(m, 200 + m, 300 + m)
    _, ids_a, ids_b = a.shared_leaves(b)
    for rooted in (False, True):
        args = ref.pair_arrays(a, b, rooted)
        got = _both(args, rooted, "m %d rooted %s" % (m, rooted))
        want = ref.compare(a, ids_a, b, ids_b, rooted)
        assert list(got[0]) == want["distance"] and list(got[2]) == want["intersection"]
        res = a.compare_clades(b, rooted=rooted, device=0)
        assert list(res.match) == want["match"] and list(res.transfer) == want["transfer"] and res.rf == want["rf"]
        # rank(m): a row against the candidate [0, m) and the candidates that end at m
        pos = args[1]
        _both((m, pos, [0, 1], [m, m], [0, m - 2, 1], [m, m, m - 1]), rooted, "rank(m) at m %d" % m)


def test_scans_of_several_words_per_thread():
    case = _levels_case(4097, 5)      # 65 words: one per thread, the last threads none
    for rooted in (False, True):
        _both(case[rooted], rooted, "m 4097 rooted %s" % rooted)
    case = _levels_case(70001, 6)      # 1094 words: five per thread
    rng = np.random.default_rng(7)
    for rooted in (False, True):
        m, pos, a_lo, a_hi, b_lo, b_hi = case[rooted]
        by_size = np.argsort(a_hi - a_lo, kind="stable")
        rows = np.unique(np.concatenate([by_size[:8], by_size[-8:], rng.choice(len(a_lo), 48, replace=False)]))[:64]
        _both((m, pos, a_lo[rows], a_hi[rows], b_lo, b_hi), rooted, "m 70001 rooted %s" % rooted)


def test_the_cap_and_the_whole_lds_budget():
    m = _capi.CLADE_MATCH_MAX_LEAVES
    case = _levels_case(m, 8)
    rng = np.random.default_rng(9)
    for rooted in (False, True):
        _, pos, a_lo, a_hi, b_lo, b_hi = case[rooted]
        by_size = np.argsort(a_hi - a_lo, kind="stable")
        rows = np.concatenate([by_size[:4], by_size[-4:], rng.choice(len(a_lo), 16, replace=False)])
        # and ranges no tree gave (any list of ranges is matched as it stands): sizes 2, 3, m / 2, m - 2, m - 1, m
        lo = np.concatenate([a_lo[rows], [0, 5, 0, m // 4, 1, 0, 1, 0]]).astype(np.int32)
        hi = np.concatenate([a_hi[rows], [2, 8, m // 2, m // 4 + m // 2, m - 1, m - 2, m, m]]).astype(np.int32)
        assert len(lo) == 32
        _both((m, pos, lo, hi, b_lo, b_hi), rooted, "the cap, rooted %s" % rooted)


def test_more_rows_than_a_chunk_and_than_the_grid():
    case = _levels_case(3000, 10)
    for rooted in (False, True):
        want = _capi.clade_match(*case[rooted], rooted=rooted, device=-1)
        assert len(want[0]) == 3000 - (2 if rooted else 3)
        for chunk in (1, 7, 0):
            _same(_capi.clade_match(*case[rooted], rooted=rooted, device=0, chunk_rows=chunk), want, "chunk_rows %d rooted %s" % (chunk, rooted))
    case = _levels_case(5000, 11)      # 4997 rows in one chunk: more than the grid's 4096 workgroups
    _both(case[False], False, "more rows than the grid")


def test_near_complement_tie_identical_trees_and_no_candidates():
    pos = np.arange(8)
    got = _both((8, pos, [0], [5], [0, 5], [3, 7]), False, "near-complement")      # {0..4}: {5,6} at m - d = 1 beats {0,1,2} at 2
    assert (got[0][0], got[1][0], got[2][0]) == (1, 1, 0)
    got = _both((8, pos, [0], [5], [0, 5], [3, 7]), True, "rooted")
    assert (got[0][0], got[1][0], got[2][0]) == (2, 0, 3)
    for b_lo, b_hi in (([1, 3], [3, 5]), ([3, 1], [5, 3])):      # {2,3} against {1,2} and {3,4}: the lower index, either way round
        got = _both((8, pos, [2], [4], b_lo, b_hi), True, "tie")
        assert (got[0][0], got[1][0], got[2][0]) == (2, 0, 1)
    # equal sizes far apart in B's list: the stable sort by size keeps the lower index in front
    b_lo = np.array([0, 2, 4, 6, 1, 3, 5] * 40, dtype=np.int32)
    got = _both((8, pos, [1, 2], [3, 4], b_lo, b_lo + 2), True, "ties in a long list")
    assert list(got[1]) == [4, 1]
    got = _both((8, pos, [2, 0], [4, 5], [], []), False, "no candidates")
    assert list(got[0]) == [-1, -1] and list(got[1]) == [-1, -1] and list(got[2]) == [0, 0]
    t = ref.random_tree(300, 12)
    for rooted in (False, True):
        res = t.compare_clades(t, rooted=rooted, device=0)
        assert res.rf == 0 and not res.distance.any() and (res.match == res.nodes).all() and (res.intersection == res.n_leaves).all()


@pytest.mark.parametrize("rooted", [False, True])
def test_balanced_against_caterpillar(rooted):
    names = ["L%d" % k for k in range(64)]
    a, b = SuchTree(synth.balanced_tree(6) + (names,)), SuchTree(synth.caterpillar_tree(64) + (names,))
    args = ref.pair_arrays(a, b, rooted)
    got = _both(args, rooted, "balanced against caterpillar")
    _, ids_a, ids_b = a.shared_leaves(b)
    want = ref.compare(a, ids_a, b, ids_b, rooted)
    assert list(got[0]) == want["distance"] and list(got[2]) == want["intersection"]
    # larger: every candidate size once, so the windows are wide index ranges
    names = ["L%d" % k for k in range(2048)]
    a, b = SuchTree(synth.balanced_tree(11) + (names,)), SuchTree(synth.caterpillar_tree(2048) + (names,))
    _both(ref.pair_arrays(a, b, rooted), rooted, "balanced against caterpillar, 2048 leaves")
    _both(ref.pair_arrays(b, a, rooted), rooted, "caterpillar against balanced, 2048 leaves")


def test_size_windows_on_and_off(monkeypatch):
    case = _levels_case(3000, 13)
    for rooted in (False, True):
        want = _capi.clade_match(*case[rooted], rooted=rooted, device=-1)
        for value in ("0", "1"):
            monkeypatch.setenv(WINDOW, value)
            _same(_capi.clade_match(*case[rooted], rooted=rooted, device=0), want, "windows %s rooted %s" % (value, rooted))
        monkeypatch.delenv(WINDOW)
        _same(_capi.clade_match(*case[rooted], rooted=rooted, device=0), want, "the default, rooted %s" % rooted)


def test_compare_clades_on_ml_against_nj(ml_arrays, nj_arrays):
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    sel = np.random.default_rng(21).choice(len(leaves1), 2000, replace=False)
    a, b = SuchTree((p1, d1)), SuchTree((p2, d2))
    for rooted in (False, True):
        host = a.compare_clades(b, leaves=(leaves1[sel], nj_of[sel]), rooted=rooted, device=None)
        dev = a.compare_clades(b, leaves=(leaves1[sel], nj_of[sel]), rooted=rooted)      # (the tree's device)
        for k in host.COLUMNS:
            assert np.array_equal(getattr(dev, k), getattr(host, k), equal_nan=True), k
        assert (dev.rf, dev.exact, dev.n_a, dev.n_b, dev.mean_transfer) == (host.rf, host.exact, host.n_a, host.n_b, host.mean_transfer)
        assert dev.n_leaves_shared == 2000 and 0 < dev.exact < dev.n_a
    assert a._dev_tree is None and b._dev_tree is None      # (parent arrays alone: neither tree was uploaded)


def test_transfer_support_equals_its_host_form():
    a = ref.random_tree(500, 14)
    reps = [ref.shuffled_tree(500, 15, 16), synth.to_newick(a._flat.parent, a._flat.distance, a.leaf_nodes), ref.shuffled_tree(500, 17, 18)]
    for rooted in (False, True):
        host = a.transfer_support(reps, rooted=rooted, device=None)
        dev = a.transfer_support(reps, rooted=rooted)
        assert dev.n_replicates == 3 and (dev.transfer_sum == host.transfer_sum).all() and (dev.exact_count == host.exact_count).all()
        assert np.array_equal(dev.support, host.support) and (dev.exact_count >= 1).all()
