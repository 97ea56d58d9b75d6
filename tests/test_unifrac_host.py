"""The host side of Faith's PD and the union sums behind UniFrac (no GPU): st_unifrac_depths(device = -1), the restatement
of the kernels' set merge, against the brute-force definition; the quantiser; invariance under range splits, chunking and
row order; a float64 cross-check on the golden linked trees; the plan under the sanitizers; argument checks of the library
and the facade.

The integer tests are exact.  Bound of the float cross-check (test_float_cross_check_on_golden_trees).  PD of a set
with t merged positions adds t float32 leaf depths and subtracts t - 1 float32 MRCA depths.  Each of these is a float32
sum of up to h_max edge lengths along one root path (h_max = edges on the deepest path), added one by one: every add
rounds once, relative 2^-24 of a partial sum that is at most max_depth, so a depth differs from the float64 sum of the
same float32 edge lengths by at most h_max 2^-24 max_depth.  Quantising a depth moves it by at most half a quantum, and
the quantum is at most 2^-39 of the largest depth: 2^-40 max_depth.  The int64 sums add nothing.  A term is therefore
off by at most e = (h_max 2^-24 + 2^-40) max_depth, and PD or a union sum by at most E(t) = (2 t - 1) e; the test allows
twice that.  UniFrac = (2 U - PD_A - PD_B) / U moves, for errors dU, dA, dB of its three sums, by at most
(2 dU + dA + dB) / U + UniFrac dU / U <= (3 E(t_U) + E(t_A) + E(t_B)) / U, UniFrac being at most 1 (first order in
d / U); the test allows twice that as well."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import unifrac_cases as uc
from conftest import ROOT, golden_path
from suchtree_amd import _capi, compare, build as st_build


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()
    return _capi.load()


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_restatement_against_brute_force(n):
    parent, depth, leaf_node, d, h, sets = uc.case(n)
    assert (d < 0).any() and len(sets) >= 5
    want_pd, want_union = uc.brute_force(parent, depth, leaf_node, sets)
    pd_q, union_q = _capi.unifrac_depths(d, h, sets)
    assert pd_q.dtype == np.int64 and len(union_q) == len(sets) * (len(sets) - 1) // 2
    assert (pd_q == want_pd).all(), np.flatnonzero(pd_q != want_pd)[:5]
    assert (union_q == want_union).all(), np.flatnonzero(union_q != want_union)[:5]
    sizes = {len(s) for s in sets}
    assert sizes >= {k for k in uc.SIZES if k <= n} | {n}


def test_quantiser():
    f = np.float32
    for top in (1.0, 1.9999999, 3.0e38, 1.0e-45, 0.75, 123456.7):
        d = np.array([top, -top / 3, 0.0], dtype=f)
        h = np.array([top / 7, -top], dtype=f)
        d_q, h_q, shift = _capi.unifrac_quantise(d, h)
        assert shift == 39 - int(np.floor(np.log2(float(f(top)))))
        assert 2 ** 39 <= max(np.abs(d_q).max(), np.abs(h_q).max()) < 2 ** 40
        for q, v in zip(list(d_q) + list(h_q), list(d) + list(h)):      # q(v) = llrint(ldexp(v, shift)): round half to even
            exact = int(np.rint(np.ldexp(np.float64(v), shift)))
            assert int(q) == exact
    zeros = _capi.unifrac_quantise(np.zeros(4, dtype=f), np.zeros(3, dtype=f))
    assert zeros[2] == 0 and not zeros[0].any() and not zeros[1].any()
    assert _capi.unifrac_quantise(np.zeros(1, dtype=f), np.zeros(0, dtype=f))[2] == 0      # one leaf: no h
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            _capi.unifrac_quantise(np.array([1.0, bad], dtype=f), np.array([0.5], dtype=f))
        with pytest.raises(ValueError):
            _capi.unifrac_quantise(np.array([1.0, 2.0], dtype=f), np.array([bad], dtype=f))
    # an explicit shift is honoured ...
    d_q, h_q, shift = _capi.unifrac_quantise(np.array([1.5, 0.25], dtype=f), np.array([0.125], dtype=f), shift=3)
    assert shift == 3 and d_q.tolist() == [12, 2] and h_q.tolist() == [1]
    assert _capi.unifrac_quantise(np.array([0.3], dtype=f), np.zeros(0, dtype=f), shift=0)[0].tolist() == [0]
    # ... up to the bound: the largest |q| allowed is 2^40 - 2^16 (a float32 below 2 at shift 39), 2^40 itself is refused
    below_two = np.nextafter(f(2.0), f(0.0))
    assert _capi.unifrac_quantise(np.array([below_two], dtype=f), np.zeros(0, dtype=f), shift=39)[0].tolist() == [2 ** 40 - 2 ** 16]
    assert _capi.unifrac_quantise(np.array([1.0], dtype=f), np.zeros(0, dtype=f), shift=39)[0].tolist() == [2 ** 39]
    for d, s in (([2.0], 39), ([1.0], 40), ([-2.0], 39), ([1.0, 1.0e-30], 256)):
        with pytest.raises(ValueError):
            _capi.unifrac_quantise(np.array(d, dtype=f), np.zeros(len(d) - 1, dtype=f), shift=s)
    with pytest.raises(ValueError):
        _capi.unifrac_quantise(np.array([1.0, 1.0], dtype=f), np.array([-2.0], dtype=f), shift=39)      # h counts as well
    for s in (-2, 257):
        with pytest.raises(ValueError):
            _capi.unifrac_quantise(np.array([1.0], dtype=f), np.zeros(0, dtype=f), shift=s)
    # st_unifrac_depths refuses what the quantiser could not have produced
    ok = np.array([2 ** 40 - 1, -(2 ** 40 - 1)], dtype=np.int64)
    assert _capi.unifrac_depths(ok, np.array([5], dtype=np.int64), [[0, 1]])[0].tolist() == [2 ** 40 - 1 - (2 ** 40 - 1) - 5]
    for d_q, h_q in (([2 ** 40, 0], [0]), ([0, -2 ** 40], [0]), ([0, 0], [2 ** 40])):
        with pytest.raises(ValueError):
            _capi.unifrac_depths(np.array(d_q, dtype=np.int64), np.array(h_q, dtype=np.int64), [[0, 1]])


def test_invariances():
    n = 200
    parent, depth, leaf_node, d, h, sets = uc.case(n)
    sets = sets[:23]
    total = len(sets) * (len(sets) - 1) // 2
    pd_q, union_q = _capi.unifrac_depths(d, h, sets)
    assert len(union_q) == total
    for cuts in ([0, total], [0, 1, total], [0, 7, 8, 100, total], [0, 3, 3, total], list(range(0, total, 37)) + [total]):
        parts = [_capi.unifrac_depths(d, h, sets, begin=a, count=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert (np.concatenate([u for _, u in parts]) == union_q).all(), cuts
        assert all((p == pd_q).all() for p, _ in parts)      # PD of every set, whatever the range
    mid = 5 * 4 // 2 + 2      # pair (i = 5, j = 2): the range starts in the middle of a row
    assert (_capi.unifrac_depths(d, h, sets, begin=mid, count=40)[1] == union_q[mid:mid + 40]).all()
    for chunk in (1, 7, 64, 0):
        got = _capi.unifrac_depths(d, h, sets, chunk_pairs=chunk)
        assert (got[0] == pd_q).all() and (got[1] == union_q).all(), chunk
    order = np.random.default_rng(3).permutation(len(sets))
    pd_r, union_r = _capi.unifrac_depths(d, h, [sets[r] for r in order])
    assert (pd_r == pd_q[order]).all()
    tri = lambda i, j: max(i, j) * (max(i, j) - 1) // 2 + min(i, j)      # noqa: E731
    k = 0
    for i in range(len(sets)):
        for j in range(i):
            assert union_r[k] == union_q[tri(order[i], order[j])]
            k += 1
    res = compare.SetUniFrac(len(sets), mid, 0, pd_q, union_q[mid:mid + 40])
    assert res.pair(0) == (5, 2) and res.pair(3) == (6, 0) and res.count == 40
    with pytest.raises(ValueError):
        res.matrix()


def _golden(which):
    import pandas as pd
    from suchtree_amd import SuchLinkedTrees, SuchTree
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("of", ["A", "B"])
def test_float_cross_check_on_golden_trees(which, of):
    """The bound: the module docstring.  Depths from the CPU oracle (float32 sums along the path, as the kernels'), the
    truth a float64 sum of the same float32 edge lengths over the nodes with a member below them."""
    from oracle.oracle import OracleTree
    slt = _golden(which)
    own, tree, root, leaves, members = slt._partner_rows(of, 1, None)
    parent, dist = np.asarray(tree._flat.parent), np.asarray(tree._flat.distance)
    univ = tree._depth_first_leaves()
    n = len(univ)
    where = np.full(tree.size, -1, dtype=np.int64)
    where[univ] = np.arange(n)
    sets = [np.sort(where[m]) for m in members]
    oracle = OracleTree(parent, dist)
    d = oracle.distances(np.stack([np.full(n, root), univ], axis=1))
    mrca = oracle.mrca_bulk(np.stack([univ[:-1], univ[1:]], axis=1)).astype(np.int64)
    h = oracle.distances(np.stack([np.full(n - 1, root), mrca], axis=1))
    assert (d.astype(np.float32) == d).all() and (h.astype(np.float32) == h).all()
    res = compare.unifrac_from_depths(d, h, sets)
    # the truth
    edge = np.where(parent >= 0, dist.astype(np.float64), 0.0)
    masks = uc.node_masks(parent, univ, sets)
    levels = np.zeros(tree.size, dtype=np.int64)
    for v in range(tree.size):
        u, k = v, 0
        while parent[u] >= 0:
            u, k = parent[u], k + 1
        levels[v] = k
    h_max, max_depth = int(levels.max()), float(d.max())
    e = (h_max * 2.0 ** -24 + 2.0 ** -40) * max_depth
    E = lambda t: (2 * t - 1) * e      # noqa: E731
    size = np.array([len(s) for s in sets])
    want_pd = masks @ edge
    worst = np.abs(res.pd - want_pd) / (2 * E(size))
    print("%s of=%s: %d sets, h_max %d, max depth %.4g, e %.3g, PD error / bound at most %.3g" % (which, of, len(sets), h_max, max_depth, e, worst.max()))
    assert (np.abs(res.pd - want_pd) <= 2 * E(size)).all()
    got, worst_u = res.unifrac, 0.0
    assert res.count == len(sets) * (len(sets) - 1) // 2
    for k in range(res.count):
        i, j = res.pair(k)
        both = masks[i] | masks[j]
        U = both @ edge
        t = len(np.union1d(sets[i], sets[j]))
        want = (2 * U - want_pd[i] - want_pd[j]) / U
        bound = 2 * (3 * E(t) + E(size[i]) + E(size[j])) / U
        worst_u = max(worst_u, abs(got[k] - want) / bound)
        assert abs(got[k] - want) <= bound, (k, i, j, got[k], want, bound)
        assert -bound <= got[k] <= 1 + bound
    print("%s of=%s: %d pairs, UniFrac error / bound at most %.3g" % (which, of, res.count, worst_u))
    M = res.matrix()
    assert (M == M.T).all() and not M.diagonal().any() and M[res.pair(1)] == got[1]
    assert list(res.to_dataframe().columns) == ["i", "j", "union", "shared", "unifrac", "phylosor"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_unifrac_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_unifrac")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_unifrac.cpp"), os.path.join(csrc, "unifrac_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize unifrac ok" in out.stdout


def _raw(d_q, h_q, n, pos, off, n_sets, begin, count, chunk, device=-1):
    L = _capi.load()
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)      # noqa: E731
    d_q, h_q, pos, off = arr(d_q, np.int64), arr(h_q, np.int64), arr(pos, np.int32), arr(off, np.int64)
    pd_q, union_q = np.zeros(max(n_sets, 1), dtype=np.int64), np.zeros(max(count, 1), dtype=np.int64)
    p = _capi._ptr
    return L.st_unifrac_depths(device, p(d_q), p(h_q), n, p(pos), 0 if pos is None else len(pos), p(off), n_sets, begin, count, chunk,
                               p(pd_q), p(union_q))


def test_library_argument_errors():
    d_q, h_q = [5, 6, 7, 8, 9], [1, 2, 3, 4]
    ok = ([0, 2, 4, 1, 3, 0], [0, 3, 5, 6])      # three sets: three pairs
    assert _raw(d_q, h_q, 5, *ok, 3, 0, 3, 0) == _capi.ST_OK
    assert _raw(d_q, h_q, 5, *ok, 3, 3, 0, 0) == _capi.ST_OK      # an empty range at the end
    assert _raw(d_q, h_q, 5, None, [0], 0, 0, 0, 0) == _capi.ST_OK      # no sets
    cases = {
        "universe of 0": (d_q, h_q, 0, *ok, 3, 0, 3, 0),
        "universe above the limit": (d_q, h_q, _capi.UNIFRAC_MAX_UNIVERSE + 1, *ok, 3, 0, 3, 0),
        "position outside": (d_q, h_q, 5, [0, 2, 5, 1, 3, 0], ok[1], 3, 0, 3, 0),
        "negative position": (d_q, h_q, 5, [-1, 2, 4, 1, 3, 0], ok[1], 3, 0, 3, 0),
        "unsorted set": (d_q, h_q, 5, [0, 4, 2, 1, 3, 0], ok[1], 3, 0, 3, 0),
        "duplicate": (d_q, h_q, 5, [0, 2, 2, 1, 3, 0], ok[1], 3, 0, 3, 0),
        "offsets go back": (d_q, h_q, 5, ok[0], [0, 3, 2, 6], 3, 0, 3, 0),
        "offsets past the positions": (d_q, h_q, 5, ok[0], [0, 3, 5, 7], 3, 0, 3, 0),
        "range past the triangle": (d_q, h_q, 5, *ok, 3, 1, 3, 0),
        "range begins past the triangle": (d_q, h_q, 5, *ok, 3, 4, 0, 0),
        "negative begin": (d_q, h_q, 5, *ok, 3, -1, 2, 0),
        "negative count": (d_q, h_q, 5, *ok, 3, 0, -1, 0),
        "negative chunk_pairs": (d_q, h_q, 5, *ok, 3, 0, 3, -1),
        "negative n_sets": (d_q, h_q, 5, *ok, -1, 0, 0, 0),
        "NULL sets": (d_q, h_q, 5, ok[0], None, 3, 0, 3, 0),
        "NULL positions": (d_q, h_q, 5, None, ok[1], 3, 0, 3, 0),
        "NULL d_q": (None, h_q, 5, *ok, 3, 0, 3, 0),
        "NULL h_q": (d_q, None, 5, *ok, 3, 0, 3, 0),
        "d_q at 2^40": ([5, 6, 1 << 40, 8, 9], h_q, 5, *ok, 3, 0, 3, 0),
        "h_q at -2^40": (d_q, [1, 2, 3, -(1 << 40)], 5, *ok, 3, 0, 3, 0),
        "device below -1": (d_q, h_q, 5, *ok, 3, 0, 3, 0, -2),
    }
    for what, args in cases.items():
        assert _raw(*args) == _capi.ST_ERR_ARG, what
        assert _capi.last_error(), what
    # the tree entry refuses its own arguments before it looks at the tree
    L, p, c = _capi.load(), _capi._ptr, _capi.ctypes
    pos, off, univ = np.array(ok[0], dtype=np.int32), np.array(ok[1], dtype=np.int64), np.arange(5, dtype=np.int64)
    pd_q, union_q, bad, used = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), c.c_int64(0), c.c_int32(0)

    def tree_call(n=5, u=univ, begin=0, count=3, shift=-1, chunk=0):
        return L.st_unifrac_host(None, 0, p(u), n, p(pos), 6, p(off), 3, begin, count, shift, chunk, p(pd_q), p(union_q), c.byref(used), None, None,
                                 c.byref(bad))
    for kw in ({"n": 2}, {"u": None}, {"count": 4}, {"shift": -2}, {"shift": 257}, {"chunk": -1}, {}):
        assert tree_call(**kw) == _capi.ST_ERR_ARG, kw
    assert "tree is NULL" in _capi.last_error()
    with pytest.raises(ValueError):
        _capi.unifrac_depths(d_q, h_q, [[0, 7]])
    with pytest.raises(ValueError):
        _capi.unifrac_depths(d_q, h_q[:3], [[0, 1]])
    with pytest.raises(ValueError):
        _capi.unifrac_depths(d_q, h_q, [[1, 0]])      # the library's own check: not increasing
    with pytest.raises(ValueError):
        _capi.unifrac_depths(d_q, h_q, [[0], [1]], begin=1, count=1)


def test_header_declares_and_capi_binds_the_exports():
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    L = _capi.load()
    for name in ("st_unifrac_host", "st_unifrac_depths", "st_unifrac_quantise"):
        assert ("int %s(" % name) in header and name in _capi.SYMBOLS and getattr(L, name).argtypes
    assert "#define ST_UNIFRAC_MAX_UNIVERSE %d\n" % _capi.UNIFRAC_MAX_UNIVERSE in header and _capi.UNIFRAC_MAX_UNIVERSE == 1 << 20
    assert "#define ST_UNIFRAC_LANE_MAX %d\n" % _capi.UNIFRAC_LANE_MAX in header


def test_facade_errors_raised_before_any_upload():
    import pandas as pd
    from suchtree_amd import SuchLinkedTrees, SuchTree, synth
    from suchtree_amd.exceptions import InvalidNodeError, NodeNotFoundError
    ta = SuchTree(synth.random_binary_tree(6, seed=1) + (["a%d" % i for i in range(6)],))
    tb = SuchTree(synth.random_binary_tree(9, seed=2) + (["b%d" % i for i in range(9)],))
    m = np.zeros((6, 9), dtype=int)
    m[0, :4] = m[1, 3:6] = m[2, 8] = 1
    slt = SuchLinkedTrees(ta, tb, pd.DataFrame(m, index=list(ta.leaves.keys()), columns=list(tb.leaves.keys())))
    for kw in ({"of": "C"}, {"min_partners": -1}, {"max_partners": 1.5}, {"begin": -1}, {"count": -1}, {"count": 4}, {"begin": 2, "count": 2},
               {"shift": -1}, {"shift": 2.5}, {"begin": True}):
        with pytest.raises(ValueError):
            slt.partner_unifrac(**kw)
    names = list(tb.leaves.keys())
    inner = next(v for v in range(tb.size) if tb._flat.left[v] != -1 and v != tb.root_node)
    for kw in ({"sets": [[names[0], names[0]]]},                              # a repeated member
               {"sets": [names], "root": inner},                               # a member that does not lie under root
               {"sets": [[tb.root_node, tb.leaves[names[0]]]]},               # an id that is no leaf
               {"sets": [[names[0]]], "chunk_pairs": -1}, {"sets": [[names[0]], [names[1]]], "begin": 2}):
        with pytest.raises(ValueError):
            tb.unifrac(**kw)
    with pytest.raises(NodeNotFoundError):
        tb.unifrac([["nobody"]])
    with pytest.raises(InvalidNodeError):
        tb.unifrac([[names[0]]], root=tb.size)
    # no row, or only empty sets: nothing is launched, and neither tree goes to a device
    none = slt.partner_unifrac(of="A", min_partners=5)
    assert len(none) == 0 and none.count == 0 and len(none.leaves) == 0 and none.names == [] and none.root == tb.root_node
    empty = tb.unifrac([[], []])
    assert empty.pd_q.tolist() == [0, 0] and empty.union_q.tolist() == [0] and np.isnan(empty.unifrac).all() and np.isnan(empty.phylosor).all()
    assert ta._dev_tree is None and tb._dev_tree is None
