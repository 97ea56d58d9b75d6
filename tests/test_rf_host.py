"""st_rf_tasks on the host (device = -1), _capi.rf_tasks, compare.tree_set and compare.rf_relabelled (CPU): the restatement
of Day's method against the set oracle of tests/rf_reference.py (Python sets, no positions and no ranges) at the edges of
the blocks of 64 positions, against the delta-0 rows of st_clade_match at several blocks and at the cap, the orientation
and range identities, the facades against transfer_support and dendrogram_congruence, every documented argument error, and
rf_plan.cpp as a program of its own under ASan + UBSan.  Every comparison is of integers and exact."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rf_reference as ref
from conftest import ROOT
from linkage_reference import random_codes
from suchtree_amd import _capi, compare, synth
from suchtree_amd.suchtree import SuchTree

EDGES = [4, 5, 63, 64, 65, 128, 129]


def _case(m, rooted):
    trees = ref.tree_set(m, 1000 + m)
    sets = [ref.clade_sets(parent, ids, rooted) for parent, ids in trees]
    return trees, sets, ref.library_sides(trees, rooted)


@pytest.mark.parametrize("rooted", [False, True])
@pytest.mark.parametrize("m", EDGES)
def test_the_host_restatement_equals_the_set_oracle(m, rooted):
    trees, sets, (where, offsets, lo, hi, sides) = _case(m, rooted)
    n = len(trees)
    assert [len(s) for s in sets] == np.diff(offsets).tolist()      # (the library's lists are distinct sets, the oracle's sets)
    assert len(sets[5]) == 0 and sets[0] == sets[1] and len(sets[2]) == (m - 2 if rooted else m - 3)
    shared, counts = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted)
    pairs = ref.triangle(n)
    assert shared.dtype == np.int32 and counts.dtype == np.int64 and len(shared) == len(pairs) == n * (n - 1) // 2
    assert shared.tolist() == [ref.shared(sets[i], sets[j]) for i, j in pairs]
    assert shared[0] == len(sets[0]) and all(shared[k] == 0 for k, (i, j) in enumerate(pairs) if 5 in (i, j))
    # how many other trees hold each clade
    freq = ref.frequencies(sets)
    want = [freq[s] - 1 for side in sides for s in ref.side_sets(side, rooted)]
    assert counts.tolist() == want
    # the ranges of the triangle concatenate to it, whatever the chunk
    cuts = [0, 1, 4, 9, len(pairs)]
    parts = [_capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, begin=b, count=e - b, want_count=False, chunk_tasks=c)[0]
             for b, e, c in zip(cuts, cuts[1:], (0, 1, 2, 5))]
    assert np.concatenate(parts).tolist() == shared.tolist()
    assert _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, begin=len(pairs), want_count=False)[0].tolist() == []
    # either direction, and a tree against itself
    ti = np.array([i for i, _ in pairs] + list(range(n)), dtype=np.int32)
    tj = np.array([j for _, j in pairs] + list(range(n)), dtype=np.int32)
    forward, c_forward = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, task_i=ti, task_j=tj)
    backward, _ = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, task_i=tj, task_j=ti, task_p=np.full(len(ti), -1), chunk_tasks=3)
    assert forward.tolist() == backward.tolist() == shared.tolist() + np.diff(offsets).tolist()
    assert c_forward.tolist() == (counts + 2).tolist()      # (a tree against itself: every clade is its own match)


@pytest.mark.parametrize("rooted", [False, True])
@pytest.mark.parametrize("m", EDGES)
def test_alignments_against_the_set_oracle(m, rooted):
    trees, sets, (where, offsets, lo, hi, _) = _case(m, rooted)
    n, rng = len(trees), np.random.default_rng(m)
    align = np.stack([np.arange(m)] + [rng.permutation(m) for _ in range(5)]).astype(np.int32)
    ti, tj, tp = (rng.integers(0, hi_, size=60).astype(np.int32) for hi_ in (n, n, len(align)))
    tp[::7] = -1
    got, _ = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, align=align, task_i=ti, task_j=tj, task_p=tp, chunk_tasks=16)
    want = [ref.shared(sets[i], sets[j], None if p < 0 else align[p], rooted) for i, j, p in zip(ti, tj, tp)]
    assert got.tolist() == want
    # the identity as a row of the table and as -1
    named = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, align=align, task_i=ti, task_j=tj, task_p=np.zeros(60, dtype=np.int32))[0]
    plain = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, task_i=ti, task_j=tj)[0]
    assert named.tolist() == plain.tolist()


def _levels_trees(m, seed, n=3):
    """n seeded random trees of m leaves as (parent, ids), the common leaves dealt to each in another order"""
    leaves = np.arange(m, dtype=np.int64) * 2
    return [(synth.random_binary_tree_levels(m, seed=seed + t)[0], leaves[np.random.default_rng(seed + 10 + t).permutation(m)] if t else leaves)
            for t in range(n)]


@pytest.mark.parametrize("m", [4097, 16384])
def test_large_trees_against_the_delta_0_rows_of_clade_match(m):
    trees = _levels_trees(m, 5 * m)
    for rooted in (False, True):
        where, offsets, lo, hi, sides = ref.library_sides(trees, rooted)
        shared, _ = _capi.rf_tasks(m, where, offsets, lo, hi, rooted=rooted, want_count=False)
        assert shared[0] < offsets[1]      # (two random trees: not everything is shared)
        for k, (i, j) in ((0, (1, 0)), (2, (2, 1))):
            pos_b = where[j][sides[i][0]]      # tree i's position -> tree j's position of the same leaf
            distance, match, _ = _capi.clade_match(m, pos_b, sides[i][2], sides[i][3], sides[j][2], sides[j][3], rooted, -1)
            assert int(((match >= 0) & (distance == 0)).sum()) == shared[k], (m, rooted, i, j)


def _newick(tree):
    return synth.to_newick(tree._flat.parent, tree._flat.distance, tree.leaf_nodes)


def test_tree_set_facade_and_transfer_support():
    from clade_match_reference import random_tree, shuffled_tree
    a = random_tree(90, 14)
    others = [shuffled_tree(90, 15, 16), _newick(a), shuffled_tree(90, 17, 18), random_tree(90, 14)]
    for rooted in (False, True):
        res = compare.tree_set([a] + others, rooted=rooted, device=None)
        assert isinstance(res, compare.TreeSetComparison) and (res.n_trees, res.n_leaves_shared, res.rooted, res.begin, res.count) == (5, 90, rooted, 0, 10)
        assert len(res) == 10 and res.pair(0) == (1, 0) and res.pair(9) == (4, 3) and sorted(res.leaves) == sorted(a.leaves)
        support = a.transfer_support(others, rooted=rooted, device=None)
        nodes, n_leaves, frequency = res.clades(0)
        assert nodes.tolist() == support.nodes.tolist() and n_leaves.tolist() == support.n_leaves.tolist()
        assert (frequency - 1).tolist() == support.exact_count.tolist() and (frequency >= 3).all()      # (two copies of a among the others)
        for k in range(10):
            i, j = res.pair(k)
            trees = [a] + [t if isinstance(t, SuchTree) else a for t in others]
            two = trees[i].compare_clades(trees[j], rooted=rooted, device=None)
            assert (res.shared[k], res.rf[k]) == (two.exact, two.rf) and res.rf_normalised[k] == two.rf_normalised
        M = res.matrix("rf")
        assert M.shape == (5, 5) and (M == M.T).all() and not M.diagonal().any() and M[2, 0] == 0 == M[4, 2] and M[1, 0] == res.rf[0]
        assert res.matrix("shared")[3, 1] == res.shared[4] and res.matrix("rf_normalised").dtype == np.float64
        part = compare.tree_set([a] + others, rooted=rooted, begin=3, count=4, device=None)
        assert part.shared.tolist() == res.shared[3:7].tolist() and part.clades(1)[2] is None and part.pair(0) == res.pair(3)
        with pytest.raises(ValueError, match="whole triangle"):
            part.matrix()
        assert compare.tree_set([a] + others, rooted=rooted, frequencies=False, device=None).clades(0)[2] is None


def test_tree_set_reads_what_it_is_given(tmp_path):
    from clade_match_reference import random_tree
    a, b = random_tree(12, 3), random_tree(16, 4)      # (L0 .. L11 are common)
    path = tmp_path / "b.nwk"
    path.write_text(_newick(b))
    dend = compare.linkage(random_codes(12, 2).astype(np.float64), device=None)
    res = compare.tree_set([a, _newick(a), str(path), b._flat], device=None)
    assert res.n_leaves_shared == 12 and res.leaves == ["L%d" % k for k in range(12)] and res.shared[0] == res.n_clades[0] == 9
    assert res.n_clades.dtype == np.int64 and res.names == ["0", "1", "2", "3"] and res.shared[5] == res.n_clades[3]
    named = compare.tree_set([dend, dend.to_flat()], leaves=[str(k) for k in range(12)], rooted=True, device=None)
    assert named.rf.tolist() == [0] and named.n_clades.tolist() == [10, 10]
    star = compare.tree_set([a, b], min_branch=1e9, device=None)      # (no branch is that long: both lists are empty)
    assert star.n_clades.tolist() == [0, 0] and star.shared.tolist() == [0] and np.isnan(star.rf_normalised[0])
    with pytest.raises(ValueError, match="tree 1 has no leaf 'L15'"):
        compare.tree_set([b, a], leaves=["L0", "L1", "L2", "L15"], device=None)
    with pytest.raises(TypeError, match="tree 1 must be"):
        compare.tree_set([a, 7], device=None)
    with pytest.raises(ValueError, match="3 common leaves"):
        compare.tree_set([a, b], leaves=["L0", "L1", "L2"], device=None)
    with pytest.raises(ValueError, match=r"pairs \[1, \+1\) of a triangle of 1"):
        compare.tree_set([a, b], begin=1, count=1, device=None)
    with pytest.raises(ValueError, match="no trees"):
        compare.tree_set([], device=None)


@pytest.mark.parametrize("min_branch", [None, 0.0])
@pytest.mark.parametrize("rooted", [True, False])
def test_rf_relabelled_is_the_rf_column_of_dendrogram_congruence(rooted, min_branch):
    n = 40
    points = np.repeat(np.random.default_rng(4).random((10, 3)), 4, axis=0)      # (ten points in four copies each: ties)
    y = np.sqrt(((points[:, None, :] - points[None, :, :]) ** 2).sum(axis=2))
    tree = compare.linkage(random_codes(n, 5).astype(np.float64), device=None).to_tree()
    ids = np.array([tree.leaves[str(i)] for i in range(n)], dtype=np.int64)
    want = compare.dendrogram_congruence(tree._flat, ids, y, rooted=rooted, min_branch=min_branch, permutations=50, seed=11, stream=2, keep_stats=True,
                                         device=None)
    d_flat = want.dendrogram.to_flat()
    d_ids = np.array([d_flat.leaves[str(i)] for i in range(n)], dtype=np.int64)
    got = compare.rf_relabelled(tree._flat, ids, d_flat, d_ids, permutations=50, seed=11, stream=2, rooted=rooted, min_branch=min_branch, device=None)
    assert got.perm_rf.dtype == np.int64 and got.perm_rf.tolist() == want.perm_rf.tolist()
    assert (got.rf, got.n_le, got.p_value) == (want.rf, want.n_le, want.p_value) and got.shared == want.exact
    assert (got.n_a, got.n_b) == (want.n_b, want.n_a) and got.rf == got.n_a + got.n_b - 2 * got.shared      # (the test's A is the dendrogram)
    longer = compare.rf_relabelled(tree._flat, ids, d_flat, d_ids, permutations=80, seed=11, stream=2, rooted=rooted, min_branch=min_branch, device=None)
    assert longer.perm_rf[:50].tolist() == got.perm_rf.tolist() and longer.rf == got.rf
    stat, p, size = got
    assert (stat, p, size) == (got.rf, got.p_value, n) and (got.permutations, got.seed, got.stream, got.rooted) == (50, 11, 2, rooted)
    none = compare.rf_relabelled(tree._flat, ids, d_flat, d_ids, permutations=0, seed=11, rooted=rooted, min_branch=min_branch, keep_stats=False, device=None)
    assert none.perm_rf is None and none.p_value == 1.0 and none.rf == got.rf


def _call(m, n_trees, where, offsets, lo, hi, unrooted=1, align=None, n_align=0, ti=None, tj=None, tp=None, n_tasks=0, begin=0, chunk=0, out=None,
          count=None, device=-1):
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    return _capi.load().st_rf_tasks(device, m, n_trees, p(where), p(offsets), p(lo), p(hi), unrooted, p(align), n_align, p(ti), p(tj), p(tp), n_tasks, begin,
                                    chunk, p(out), p(count))


def test_every_documented_argument_error():
    i32 = lambda *v: np.array(v, dtype=np.int32)      # noqa: E731
    where = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 0, 3, 2, 4]], dtype=np.int32)
    offsets = np.array([0, 2, 2, 4], dtype=np.int64)
    lo, hi = i32(0, 2, 1, 3), i32(2, 5, 3, 5)
    out, count = np.full(3, -7, dtype=np.int32), np.full(4, -7, dtype=np.int64)
    ok = dict(m=5, n_trees=3, where=where, offsets=offsets, lo=lo, hi=hi, n_tasks=3, out=out, count=count)
    ARG, BOUNDS, err = _capi.ST_ERR_ARG, _capi.ST_ERR_BOUNDS, _capi.last_error

    def bad(code, text, **kw):
        out[:], count[:] = -7, -7
        assert _call(**dict(ok, **kw)) == code and text in err(), (kw, err())
        assert (out == -7).all() and (count == -7).all()      # (nothing is written)
    assert _call(**ok) == _capi.ST_OK and out.tolist() == [0, 0, 0] and count.tolist() == [0, 0, 0, 0]
    bad(ARG, "a list of 3 leaves: 4 to 16384", m=3)
    bad(ARG, "a list of 16385 leaves", m=16385)
    bad(ARG, "negative size", n_trees=-1)
    bad(ARG, "negative size", n_align=-1)
    bad(ARG, "negative size", n_tasks=-1)
    bad(ARG, "begin < 0", begin=-1)
    bad(ARG, "chunk_tasks < 0", chunk=-1)
    bad(ARG, "where or clade_offsets is NULL", where=None)
    bad(ARG, "where or clade_offsets is NULL", offsets=None)
    bad(ARG, "align is NULL", n_align=1)
    bad(ARG, "lo or hi is NULL", lo=None)
    bad(ARG, "clade_offsets[0] = 1", offsets=np.array([1, 2, 2, 4], dtype=np.int64))
    bad(ARG, "clade_offsets[2] = 1", offsets=np.array([0, 2, 1, 4], dtype=np.int64))
    bad(ARG, "clade_offsets[3] = 4294967296", offsets=np.array([0, 2, 2, 1 << 32], dtype=np.int64))
    bad(ARG, "where[1][3] = 3: every row of where must be a permutation", where=np.array([[0, 1, 2, 3, 4], [4, 3, 2, 3, 0], [1, 0, 3, 2, 4]], dtype=np.int32))
    bad(ARG, "where[2][0] = 5", where=np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [5, 0, 3, 2, 4]], dtype=np.int32))
    bad(ARG, "where[0][4] = -1", where=np.array([[0, 1, 2, 3, -1], [4, 3, 2, 1, 0], [1, 0, 3, 2, 4]], dtype=np.int32))
    bad(ARG, "tree 2, range 1: [3, 6) of 5 positions", hi=i32(2, 5, 3, 6))
    bad(ARG, "tree 0, range 0: [2, 2) of 5 positions", lo=i32(2, 2, 1, 3))
    bad(ARG, "tree 0, range 1: [-1, 5)", lo=i32(0, -1, 1, 3))
    bad(ARG, "align[1][2] = 0: every row of align must be a permutation", align=np.array([[0, 1, 2, 3, 4], [0, 1, 0, 3, 4]], dtype=np.int32), n_align=2)
    bad(ARG, "pairs [1, +3) of a triangle of 3", begin=1)
    bad(ARG, "pairs [0, +4) of a triangle of 3", n_tasks=4, out=np.zeros(4, dtype=np.int32))
    bad(ARG, "task_p without task_i and task_j", tp=i32(0, 0, 0))
    bad(ARG, "task_i or task_j is NULL", ti=i32(0, 1, 2))
    bad(ARG, "begin = 2 with explicit tasks", ti=i32(0, 1, 2), tj=i32(0, 1, 2), begin=2)
    bad(BOUNDS, "task 1: trees (3, 0) of 3", ti=i32(0, 3, 2), tj=i32(0, 0, 0))
    bad(BOUNDS, "task 2: trees (2, -1) of 3", ti=i32(0, 1, 2), tj=i32(0, 0, -1))
    bad(BOUNDS, "task 0: alignment 0 of 0", ti=i32(0, 1, 2), tj=i32(0, 0, 0), tp=i32(0, -1, -1))
    bad(BOUNDS, "task 1: alignment -2 of 0", ti=i32(0, 1, 2), tj=i32(0, 0, 0), tp=i32(-1, -2, -1))
    bad(ARG, "out_shared is NULL", out=None)
    bad(ARG, "tasks without trees", n_trees=0)
    assert _call(**dict(ok, device=-2)) == ARG
    # no tasks: nothing to do, and the counts are zeros; out_count may be NULL
    assert _call(**dict(ok, n_tasks=0, out=None)) == _capi.ST_OK and count.tolist() == [0, 0, 0, 0]
    assert _call(**dict(ok, count=None)) == _capi.ST_OK and out.tolist() == [0, 0, 0]
    # the binding's own words
    with pytest.raises(ValueError, match="at most 16384"):
        _capi.rf_tasks(16385, where, offsets, lo, hi)
    with pytest.raises(ValueError, match="where must be"):
        _capi.rf_tasks(4, where, offsets, lo, hi)
    with pytest.raises(ValueError, match="clade_offsets end at 4, lo and hi hold 3"):
        _capi.rf_tasks(5, where, offsets, lo[:3], hi[:3])
    with pytest.raises(ValueError, match="come together"):
        _capi.rf_tasks(5, where, offsets, lo, hi, task_i=[0])
    with pytest.raises(ValueError, match="triangle of 3"):
        _capi.rf_tasks(5, where, offsets, lo, hi, begin=2, count=2)
    with pytest.raises(IndexError, match="task 0: trees"):
        _capi.rf_tasks(5, where, offsets, lo, hi, task_i=[3], task_j=[0])
    with pytest.raises(ValueError, match="chunk_tasks < 0"):
        _capi.rf_tasks(5, where, offsets, lo, hi, chunk_tasks=-1)


def test_a_list_that_repeats_a_set_counts_towards_its_first():
    # tree 0 lists [1, 3) twice; unrooted [0, 3) and [3, 5) are one bipartition and the key of both is [3, 5)
    where = np.array([[0, 1, 2, 3, 4], [0, 1, 2, 3, 4]], dtype=np.int32)
    offsets = np.array([0, 4, 6], dtype=np.int64)
    lo, hi = np.array([1, 1, 3, 0, 1, 0], dtype=np.int32), np.array([3, 3, 5, 3, 3, 3], dtype=np.int32)
    shared, counts = _capi.rf_tasks(5, where, offsets, lo, hi, rooted=False, task_i=[0], task_j=[1])
    assert shared.tolist() == [2] and counts.tolist() == [1, 0, 1, 0, 1, 1]
    shared, counts = _capi.rf_tasks(5, where, offsets, lo, hi, rooted=True, task_i=[0], task_j=[1])
    assert shared.tolist() == [2] and counts.tolist() == [1, 0, 0, 1, 1, 1]
    # the other way round every entry of tree 0's list is a clade of tree 1
    shared, counts = _capi.rf_tasks(5, where, offsets, lo, hi, rooted=False)
    assert shared.tolist() == [4] and counts.tolist() == [1, 1, 1, 1, 2, 2]
    # everything and nothing: unrooted [0, 5) is the empty side [5, 5)
    lo, hi = np.array([0, 0], dtype=np.int32), np.array([5, 5], dtype=np.int32)
    for rooted in (False, True):
        assert _capi.rf_tasks(5, where, np.array([0, 1, 2]), lo, hi, rooted=rooted)[0].tolist() == [1]


def test_the_symbol_is_declared_and_exported():
    assert "st_rf_tasks" in _capi.SYMBOLS and hasattr(_capi.load(), "st_rf_tasks")
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    assert "int st_rf_tasks(int device" in header and "#define ST_API_VERSION 7" in header and "#define ST_RF_MAX_LEAVES 16384" in header
    assert _capi.RF_MAX_LEAVES == 16384 == _capi.LINKAGE_MAX_OBJECTS and _capi.API_VERSION == 7
    assert isinstance(ctypes.c_int32(compare.RF_DEVICE_MIN_WORK).value, int)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rf_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_rf")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_rf.cpp"), os.path.join(csrc, "rf_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize rf ok" in out.stdout
