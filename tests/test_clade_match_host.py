"""The host side of the clade matching behind Robinson-Foulds and transfer support (no GPU): st_clade_ranges and
st_clade_match(device = -1) against the brute-force set reference (clade_match_reference.py), the theorems the
definitions imply, ties and empty lists, min_branch, nodes=, transfer_support, every argument error, and the plan unit
under the sanitizers.  Everything is an integer: all comparisons are exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import clade_match_reference as ref
from conftest import ROOT, golden_path
from suchtree_amd import _capi, compare, synth, build as st_build
from suchtree_amd.exceptions import InvalidNodeError
from suchtree_amd.suchtree import SuchTree

COLUMNS = ("nodes", "n_leaves", "match", "distance", "intersection", "transfer")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()
    return _capi.load()


def _assert_equals_reference(a, b, rooted, names=None):
    if names is None:
        _, ids_a, ids_b = a.shared_leaves(b)
    else:
        ids_a, ids_b = a._name_ids(names), b._name_ids(names)
    want = ref.compare(a, ids_a, b, ids_b, rooted)
    got = a.compare_clades(b, leaves=names, rooted=rooted, device=None)
    for k in COLUMNS:
        assert list(getattr(got, k)) == want[k], (k, rooted)
    assert np.allclose(got.support, want["support"], rtol=0, atol=1e-15)
    assert (got.n_a, got.n_b, got.exact, got.rf) == (want["n_a"], want["n_b"], want["exact"], want["rf"])
    assert got.n_leaves_shared == len(ids_a) and got.rooted == rooted
    # the ranges themselves
    for tree, ids in ((a, ids_a), (b, ids_b)):
        lo, hi, node = ref.ranges(tree, ids, rooted)
        order, got_node, got_lo, got_hi = _capi.clade_ranges(tree._flat.parent, ids, rooted)
        assert (got_node == node).all() and (got_lo == lo).all() and (got_hi == hi).all()
        position = ref.depth_first_positions(tree, ids)
        assert [position[int(k)] for k in order] == list(range(len(ids)))
    return got


@pytest.mark.parametrize("rooted", [False, True])
def test_golden_tree_against_itself(rooted):
    t = SuchTree(golden_path("test.tree"))
    got = _assert_equals_reference(t, t, rooted)
    assert got.rf == 0 and not got.distance.any() and (got.match == got.nodes).all() and (got.support == 1).all()
    assert got.n_a == t.num_leaves - (2 if rooted else 3)


@pytest.mark.parametrize("rooted", [False, True])
def test_gopher_against_relabelled_gopher(rooted):
    a = SuchTree(golden_path("gopher_louse/gopher.tree"))
    names = sorted(a.leaves)
    shuffled = dict(zip(names, np.random.default_rng(5).permutation(names)))
    parent, distance = a._flat.parent, a._flat.distance
    b = SuchTree((parent, distance, [str(shuffled[name]) for _, name in sorted(a.leaf_nodes.items())]))
    got = _assert_equals_reference(a, b, rooted)
    assert got.rf > 0


@pytest.mark.parametrize("rooted", [False, True])
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 128, 129])
def test_random_trees_against_reference(n, rooted):
    _assert_equals_reference(ref.random_tree(n, 100 + n), ref.shuffled_tree(n, 200 + n, 300 + n), rooted)


@pytest.mark.parametrize("rooted", [False, True])
def test_strict_subset_collapses_nodes(rooted):
    a, b = ref.random_tree(90, 11), ref.shuffled_tree(90, 12, 13)
    names = ["L%d" % k for k in np.random.default_rng(14).permutation(90)[:37]]
    got = _assert_equals_reference(a, b, rooted, names)
    assert got.n_a == 37 - (2 if rooted else 3)      # (binary: 36 MRCAs of the 37 leaves; far fewer than a's 89 nodes)
    # trees that share only some names: leaves=None is the shared ones
    c = SuchTree(synth.random_binary_tree(60, seed=15) + (["L%d" % k for k in range(40, 100)],))
    assert a.compare_clades(c, rooted=rooted, device=None).n_leaves_shared == 50
    _assert_equals_reference(a, c, rooted)


def _swap_one(parent):
    """One nearest-neighbour interchange on a copy of the parent array: an internal non-root node v with an internal
    child c swaps c's sibling-in-v with v's sibling."""
    parent = np.array(parent)
    kids = {}
    for v, p in enumerate(parent):
        kids.setdefault(int(p), []).append(v)
    for v in range(len(parent)):
        p = int(parent[v])
        if p < 0 or v not in kids:
            continue
        inner = [c for c in kids[v] if c in kids]
        if not inner or int(parent[p]) < 0:
            continue
        moved = [c for c in kids[v] if c != inner[0]][0]
        sibling = [c for c in kids[p] if c != v][0]
        parent[moved], parent[sibling] = p, v
        return parent
    raise AssertionError("no interior edge")


@pytest.mark.parametrize("rooted", [False, True])
def test_one_interchange_is_rf_two(rooted):
    parent, distance = synth.random_binary_tree(40, seed=21)
    names = ["L%d" % k for k in range(40)]
    a = SuchTree((parent, distance, names))
    moved = _swap_one(parent)
    leaf = [v for v in range(len(parent)) if v not in set(moved.tolist())]
    # (the swapped array is no longer numbered in order: the range builder takes any parent array)
    ids = np.array(leaf, dtype=np.int64)
    side_a, side_b = compare.clade_side(a._flat, ids, rooted), _capi.clade_ranges(moved, ids, rooted)
    m = len(ids)
    where_b = np.empty(m, dtype=np.int32)
    where_b[side_b[0]] = np.arange(m)
    got = compare.CladeMatches(m, rooted, side_a, side_b,
                               *_capi.clade_match(m, where_b[side_a[0]], side_a[2], side_a[3], side_b[2], side_b[3], rooted))
    assert got.rf == 2 and got.exact == got.n_a - 1 and (got.distance > 0).sum() == 1


@pytest.mark.parametrize("rooted", [False, True])
def test_balanced_against_caterpillar(rooted):
    names = ["L%d" % k for k in range(64)]
    a = SuchTree(synth.balanced_tree(6) + (names,))
    b = SuchTree(synth.caterpillar_tree(64) + (names,))
    got = _assert_equals_reference(a, b, rooted)
    # the caterpillar's clades are the prefixes {L0 .. Lk}: of the balanced tree's clades only its own prefixes are there
    # (sizes 2, 4, 8, 16, 32), and unrooted also those whose complement is a prefix: {L48 ..}, {L56 ..}, {L60 ..}, {L62, L63}
    assert got.exact == (5 if rooted else 9) and got.n_b == (62 if rooted else 61)


def test_unrooted_rows_of_a_binary_tree():
    for n, seed in ((16, 1), (33, 2), (64, 3)):
        t = ref.random_tree(n, seed)
        kids = t.get_children(t.root_node)
        if any(t.is_leaf(c) for c in kids):
            continue
        assert t.compare_clades(t, device=None).n_a == n - 3
        assert t.compare_clades(t, rooted=True, device=None).n_a == n - 2
    names = ["L%d" % k for k in range(32)]
    t = SuchTree(synth.balanced_tree(5) + (names,))      # (the root's two children are internal)
    got = t.compare_clades(t, device=None)
    assert got.n_a == 32 - 3 and sorted(got.n_leaves)[-1] == 16 and list(got.n_leaves).count(16) == 1


def test_tie_goes_to_the_lower_index_and_no_candidates():
    pos = np.arange(8)
    # {2,3} against {1,2} and {3,4}: both at 2; then the two candidates the other way round
    d, mt, i = _capi.clade_match(8, pos, [2], [4], [1, 3], [3, 5], rooted=True)
    assert (d[0], mt[0], i[0]) == (2, 0, 1)
    d, mt, i = _capi.clade_match(8, pos, [2], [4], [3, 1], [5, 3], rooted=True)
    assert (d[0], mt[0], i[0]) == (2, 0, 1)
    # unrooted, a near-complement wins: {0..4} against {5,6} (d = 7, m - d = 1) and {0,1,2} (d = 2)
    d, mt, i = _capi.clade_match(8, pos, [0], [5], [0, 5], [3, 7], rooted=False)
    assert (d[0], mt[0], i[0]) == (1, 1, 0)
    d, mt, i = _capi.clade_match(8, pos, [0], [5], [0, 5], [3, 7], rooted=True)
    assert (d[0], mt[0], i[0]) == (2, 0, 3)
    d, mt, i = _capi.clade_match(8, pos, [2, 0], [4, 5], [], [], rooted=False)
    assert list(d) == [-1, -1] and list(mt) == [-1, -1] and list(i) == [0, 0]
    none = (np.zeros(0, np.int32),) * 4
    side_a = (pos.astype(np.int32), np.array([9, 11], np.int32), np.array([2, 0], np.int32), np.array([4, 5], np.int32))
    res = compare.CladeMatches(8, False, side_a, none, d, mt, i)
    assert list(res.support) == [0, 0] and list(res.transfer) == [1, 2] and list(res.match) == [-1, -1]
    assert (res.n_b, res.exact, res.rf) == (0, 0, 2) and np.isnan(res.jaccard).all()
    assert _capi.clade_match(8, pos, [], [], [1], [3])[0].shape == (0,)


def test_min_branch_removes_the_resolved_polytomy():
    t = SuchTree("((a:1,b:1,c:1):1,(d:1,e:1):1,f:1);")
    eps = t.polytomy_epsilon
    every = t.compare_clades(t, rooted=True, device=None)
    real = t.compare_clades(t, rooted=True, min_branch=eps, device=None)
    assert len(every) == 4 and len(real) == 2      # {a,b,c} and {d,e}; the two epsilon nodes went, from both lists
    assert sorted(real.n_leaves) == [2, 3] and real.n_b == 2 and real.rf == 0
    gone = sorted(set(every.nodes) - set(real.nodes))
    assert all(t._flat.distance[v] <= eps for v in gone) and all(t._flat.distance[v] > eps for v in real.nodes)
    # against a tree that resolves the polytomy another way: only the real clades count
    u = SuchTree("(((a:1,c:1):0.5,b:1):1,(d:1,e:1):1,f:1);")
    assert t.compare_clades(u, rooted=True, min_branch=eps, device=None).exact == 2
    assert t.compare_clades(u, rooted=True, device=None).rf > 0
    assert len(t.compare_clades(t, rooted=True, min_branch=10.0, device=None)) == 0


def test_nodes_restricts_rows_not_rf():
    a, b = ref.random_tree(50, 31), ref.shuffled_tree(50, 32, 33)
    full = a.compare_clades(b, device=None)
    pick = [int(full.nodes[7]), int(full.nodes[2])]
    part = a.compare_clades(b, nodes=pick, device=None)
    assert list(part.nodes) == pick and len(part) == 2
    assert (part.rf, part.exact, part.n_a, part.n_b, part.mean_transfer) == (full.rf, full.exact, full.n_a, full.n_b, full.mean_transfer)
    assert part.row(pick[0]) == full.row(pick[0]) and part.row(pick[0])["node"] == pick[0]
    with pytest.raises(ValueError):
        a.compare_clades(b, nodes=[a.root_node], device=None)
    with pytest.raises(KeyError):
        part.row(int(full.nodes[0]))
    pd = pytest.importorskip("pandas")
    assert list(full.to_dataframe().columns) == list(compare.CladeMatches.COLUMNS) and isinstance(full.to_dataframe(), pd.DataFrame)


@pytest.mark.parametrize("rooted", [False, True])
def test_transfer_support_is_the_mean_of_the_replicates(rooted, tmp_path):
    a = ref.random_tree(30, 41)
    reps = [ref.shuffled_tree(30, 42 + r, 50 + r) for r in range(3)] + [a]
    text = synth.to_newick(reps[1]._flat.parent, reps[1]._flat.distance, reps[1].leaf_nodes)
    path = tmp_path / "rep.tree"
    path.write_text(text)
    got = a.transfer_support([reps[0], text, reps[2], a, str(path)], rooted=rooted, device=None)
    each = [a.compare_clades(r, rooted=rooted, device=None) for r in (reps[0], reps[1], reps[2], a, reps[1])]
    assert got.n_replicates == 5 and (got.nodes == each[0].nodes).all()
    assert (got.transfer_sum == sum(e.transfer for e in each)).all() and got.transfer_sum.dtype == np.int64
    assert (got.exact_count == sum((e.distance == 0).astype(int) for e in each)).all() and got.exact_count.min() >= 1
    assert np.allclose(got.support, np.mean([e.support for e in each], axis=0), rtol=0, atol=1e-12)
    assert a.transfer_support([], device=None).n_replicates == 0
    with pytest.raises(ValueError, match="L29"):
        a.transfer_support([ref.random_tree(29, 1)], device=None)
    with pytest.raises(TypeError):
        a.transfer_support([7], device=None)
    some = ["L%d" % k for k in range(0, 30, 2)]
    sub = a.transfer_support([reps[0]], leaves=some, rooted=rooted, device=None)
    assert (sub.transfer_sum == a.compare_clades(reps[0], leaves=some, rooted=rooted, device=None).transfer).all()


def _raw_match(m, pos, a_lo, a_hi, n_a, b_lo, b_hi, n_b, chunk=0, device=-1, outs=True):
    L = _capi.load()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    pos, a_lo, a_hi, b_lo, b_hi = arr(pos), arr(a_lo), arr(a_hi), arr(b_lo), arr(b_hi)
    out = [np.zeros(max(n_a, 1), np.int32) if outs else None for _ in range(3)]
    p = _capi._ptr
    return L.st_clade_match(device, m, p(pos), p(a_lo), p(a_hi), n_a, p(b_lo), p(b_hi), n_b, 1, chunk, p(out[0]), p(out[1]), p(out[2]))


def test_match_argument_errors():
    pos, lo, hi = [0, 1, 2, 3], [0], [2]
    assert _raw_match(4, pos, lo, hi, 1, lo, hi, 1) == _capi.ST_OK
    bad = [
        (3, pos[:3], lo, hi, 1, lo, hi, 1),                     # m below 4
        (_capi.CLADE_MATCH_MAX_LEAVES + 1, pos, lo, hi, 1, lo, hi, 1),
        (4, pos, lo, hi, -1, lo, hi, 1),                        # negative counts
        (4, pos, lo, hi, 1, lo, hi, -1),
        (4, None, lo, hi, 1, lo, hi, 1),                        # NULL arrays
        (4, pos, None, hi, 1, lo, hi, 1),
        (4, pos, lo, hi, 1, None, hi, 1),
        (4, [0, 1, 1, 3], lo, hi, 1, lo, hi, 1),                # not a permutation
        (4, [0, 1, 2, 4], lo, hi, 1, lo, hi, 1),
        (4, [0, -1, 2, 3], lo, hi, 1, lo, hi, 1),
        (4, pos, [2], [2], 1, lo, hi, 1),                       # lo < hi
        (4, pos, lo, hi, 1, [3], [2], 1),
        (4, pos, [-1], hi, 1, lo, hi, 1),                       # inside [0, m]
        (4, pos, lo, hi, 1, lo, [5], 1),
    ]
    for args in bad:
        assert _raw_match(*args) == _capi.ST_ERR_ARG, args
        assert _capi.last_error()
    assert _raw_match(4, pos, lo, hi, 1, lo, hi, 1, chunk=-1) == _capi.ST_ERR_ARG
    assert _raw_match(4, pos, lo, hi, 1, lo, hi, 1, device=-2) == _capi.ST_ERR_ARG
    assert _raw_match(4, pos, lo, hi, 1, lo, hi, 1, outs=False) == _capi.ST_ERR_ARG
    assert _raw_match(4, pos, None, None, 0, lo, hi, 1, outs=False) == _capi.ST_OK      # no rows: nothing is written
    with pytest.raises(ValueError):
        _capi.clade_match(4, pos, lo, hi, lo, hi, chunk_rows=-1)
    with pytest.raises(ValueError):
        _capi.clade_match(5, pos, lo, hi, lo, hi)


def test_ranges_argument_errors():
    parent = np.array([4, 4, 5, 5, 6, 6, -1], dtype=np.int32)
    order, node, lo, hi = _capi.clade_ranges(parent, [0, 1, 2, 3])
    assert list(order) == [0, 1, 2, 3] and (list(node), list(lo), list(hi)) == ([4], [0], [2])
    assert list(_capi.clade_ranges(parent, [3, 1, 2, 0], rooted=True)[0]) == [3, 1, 2, 0]
    assert list(_capi.clade_ranges(parent, [0, 1, 2, 3], rooted=True)[1]) == [4, 5]
    with pytest.raises(InvalidNodeError):
        _capi.clade_ranges(parent, [0, 1, 2, 7])
    with pytest.raises(InvalidNodeError):
        _capi.clade_ranges(parent, [0, 1, 2, -1])
    with pytest.raises(ValueError, match="not a leaf"):
        _capi.clade_ranges(parent, [0, 1, 2, 4])
    with pytest.raises(ValueError, match="twice"):
        _capi.clade_ranges(parent, [0, 1, 2, 2])
    with pytest.raises(ValueError):
        _capi.clade_ranges(parent, [0, 1, 2])
    with pytest.raises(ValueError):
        _capi.clade_ranges(parent, np.zeros(_capi.CLADE_MATCH_MAX_LEAVES + 1, dtype=np.int64))
    a = ref.random_tree(8, 1)
    with pytest.raises(ValueError):
        a.compare_clades(ref.random_tree(3, 1), device=None)      # three shared leaves
    with pytest.raises(ValueError):
        a.compare_clades(a, leaves=(np.array([0, 2, 4, 6]), np.array([0, 2, 4])), device=None)
    with pytest.raises(ValueError):
        a.compare_clades(a, leaves=(np.array([0, 2, 4, 5]), np.array([0, 2, 4, 6])), device=None)      # 5 is no leaf


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_clade_match_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_clade_match")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_clade_match.cpp"), os.path.join(csrc, "clade_match_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize clade match ok" in out.stdout
