"""Faith's PD and the union sums under the taxa-labels null on the host (st_unifrac_null_depths, device = -1), without a GPU.

Every expectation is composed from calls that exist without the feature (tests/unifrac_null_reference.py): sigma from
compare.hommola_permutation on the host, the relabelled sets sorted with numpy, _capi.unifrac_depths(device=-1) on them --
itself pinned to brute force in tests/test_unifrac_host.py.  All comparisons are exact integer equality.  Then the
invariances of the contract, the argument errors in their order, the header and the binding, the facade's errors before any
upload, compare.SetUniFracNull on a hand-made integer block, and the plan under the sanitizers as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import unifrac_cases as uc
import unifrac_null_reference as ref
from conftest import ROOT
from suchtree_amd import _capi, compare, build as st_build

SIZES = (0, 1, 2, 33, 64, 65)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    st_build.build()
    return _capi.load()


@pytest.mark.parametrize("perms", [0, 1, 5])
@pytest.mark.parametrize("n", [3, 64, 65, 300])
def test_restatement_equals_the_composition(n, perms):
    _, _, _, d, h, _ = uc.case(n)      # a tree's depths, negative ones among them
    sets = ref.sized_sets(n, SIZES, 50 + n)
    assert {len(s) for s in sets} >= {k for k in SIZES if k <= n} | {n}
    assert any(a is not b and len(a) > 1 and np.array_equal(a, b) for a in sets for b in sets)      # two identical sets
    total = len(sets) * (len(sets) - 1) // 2
    for begin, count in ((0, total), (2, total - 4)):      # the second range starts inside row 2 and ends inside the last row
        want_pd, want_union = ref.compose(d, h, sets, perms, 9 + n, 4, begin, count)
        pd_q, union_q = _capi.unifrac_null_depths(d, h, sets, begin, count, perms, 9 + n, 4)
        assert pd_q.dtype == np.int64 and pd_q.shape == (len(sets), perms + 1) and union_q.shape == (count, perms + 1)
        assert (pd_q == want_pd).all(), np.argwhere(pd_q != want_pd)[:5]
        assert (union_q == want_union).all(), np.argwhere(union_q != want_union)[:5]
    if perms:
        assert (pd_q[:, 1] != pd_q[:, 0]).any() or n == 3      # a draw differs from the observation
        whole = [r for r, s in enumerate(sets) if len(s) == n]
        assert (pd_q[whole] == pd_q[whole][:, :1]).all()      # the whole universe relabels to itself


def test_invariances():
    n = 300
    d, h = ref.depths(n, 1)
    sets = ref.sized_sets(n, SIZES, 2)
    total = len(sets) * (len(sets) - 1) // 2
    pd_q, union_q = _capi.unifrac_null_depths(d, h, sets, permutations=5, seed=77, stream=12)
    for chunk in (1, 7, 0):
        a, b = _capi.unifrac_null_depths(d, h, sets, permutations=5, seed=77, stream=12, chunk_tasks=chunk)
        assert (a == pd_q).all() and (b == union_q).all(), chunk
    # column p is the same for any permutations >= p
    a, b = _capi.unifrac_null_depths(d, h, sets, permutations=20, seed=77, stream=12)
    assert (a[:, :6] == pd_q).all() and (b[:, :6] == union_q).all()
    # column 0 is the call without a null
    pd0, union0 = _capi.unifrac_depths(d, h, sets)
    assert (pd_q[:, 0] == pd0).all() and (union_q[:, 0] == union0).all()
    # a set's and a pair's columns do not depend on the other sets or on where the set stands
    order = np.random.default_rng(3).permutation(len(sets))
    extra = [np.array([5, 9, 200]), np.arange(10, 150)]
    moved = [sets[r] for r in order] + extra
    a, b = _capi.unifrac_null_depths(d, h, moved, permutations=5, seed=77, stream=12)
    assert (a[: len(sets)] == pd_q[order]).all()
    for k in range(total):
        i, j = compare.SetUniFrac._rows(np.array([k]))
        x, y = sorted((int(np.flatnonzero(order == i[0])[0]), int(np.flatnonzero(order == j[0])[0])))
        assert (b[y * (y - 1) // 2 + x] == union_q[k]).all(), k
    # seed and stream matter; either output alone is the same
    other = _capi.unifrac_null_depths(d, h, sets, permutations=5, seed=78, stream=12)[0]
    assert (other[:, 0] == pd_q[:, 0]).all() and (other[:, 1:] != pd_q[:, 1:]).any()
    assert (_capi.unifrac_null_depths(d, h, sets, permutations=5, seed=77, stream=13)[1][:, 1:] != union_q[:, 1:]).any()
    a, none = _capi.unifrac_null_depths(d, h, sets, permutations=5, seed=77, stream=12, union=False)
    assert none is None and (a == pd_q).all()
    none, b = _capi.unifrac_null_depths(d, h, sets, 3, 11, 5, 77, 12, pd=False)
    assert none is None and (b == union_q[3:14]).all()


def _raw(d_q, h_q, n, pos, off, n_sets, begin, count, perms=2, stream=0, chunk=0, device=-1):
    L = _capi.load()
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)      # noqa: E731
    d_q, h_q, pos, off = arr(d_q, np.int64), arr(h_q, np.int64), arr(pos, np.int32), arr(off, np.int64)
    R = min(max(perms, 0), 16) + 1      # (a larger count is refused before anything is written)
    pd_q, union_q = np.zeros(max(n_sets, 1) * R, dtype=np.int64), np.zeros(max(count, 1) * R, dtype=np.int64)
    p = _capi._ptr
    return L.st_unifrac_null_depths(device, p(d_q), p(h_q), n, p(pos), 0 if pos is None else len(pos), p(off), n_sets, begin, count, perms, 5,
                                    stream, chunk, p(pd_q), p(union_q))


def test_library_argument_errors_in_their_order():
    d_q, h_q = [5, 6, 7, 8, 9], [1, 2, 3, 4]
    ok = ([0, 2, 4, 1, 3, 0], [0, 3, 5, 6])      # three sets: three pairs
    assert _raw(d_q, h_q, 5, *ok, 3, 0, 3) == _capi.ST_OK
    assert _raw(d_q, h_q, 5, *ok, 3, 3, 0) == _capi.ST_OK      # an empty range at the end
    assert _raw(d_q, h_q, 5, None, [0], 0, 0, 0) == _capi.ST_OK      # no sets
    bad_pos = [0, 2, 5, 1, 3, 0]
    cases = {
        "universe of 2": ((d_q[:2], h_q[:1], 2, *ok, 3, 0, 3), "universe"),
        "universe above the limit": ((d_q, h_q, _capi.HOMMOLA_MAX_UNIVERSE + 1, *ok, 3, 0, 3), "universe"),
        "negative permutations": ((d_q, h_q, 5, *ok, 3, 0, 3, -1), "permutations"),
        "negative stream": ((d_q, h_q, 5, *ok, 3, 0, 3, 2, -1), "stream"),
        "negative chunk_tasks": ((d_q, h_q, 5, *ok, 3, 0, 3, 2, 0, -1), "chunk_tasks"),
        "position outside": ((d_q, h_q, 5, bad_pos, ok[1], 3, 0, 3), "outside the universe"),
        "unsorted set": ((d_q, h_q, 5, [0, 4, 2, 1, 3, 0], ok[1], 3, 0, 3), "increasing"),
        "duplicate": ((d_q, h_q, 5, [0, 2, 2, 1, 3, 0], ok[1], 3, 0, 3), "increasing"),
        "offsets go back": ((d_q, h_q, 5, ok[0], [0, 3, 2, 6], 3, 0, 3), "offsets"),
        "offsets past the positions": ((d_q, h_q, 5, ok[0], [0, 3, 5, 7], 3, 0, 3), "offsets"),
        "negative n_sets": ((d_q, h_q, 5, *ok, -1, 0, 0), "negative size"),
        "NULL sets": ((d_q, h_q, 5, ok[0], None, 3, 0, 3), "NULL"),
        "NULL positions": ((d_q, h_q, 5, None, ok[1], 3, 0, 3), "offsets"),      # (n_pos goes as 0 with it)
        "range past the triangle": ((d_q, h_q, 5, *ok, 3, 1, 3), "triangle"),
        "range begins past the triangle": ((d_q, h_q, 5, *ok, 3, 4, 0), "triangle"),
        "negative begin": ((d_q, h_q, 5, *ok, 3, -1, 2), "negative"),
        "negative count": ((d_q, h_q, 5, *ok, 3, 0, -1), "negative"),
        "2^40 values": ((d_q, h_q, 5, *ok, 3, 0, 3, (1 << 40) // 3), "2^40"),
        "NULL d_q": ((None, h_q, 5, *ok, 3, 0, 3), "NULL"),
        "NULL h_q": ((d_q, None, 5, *ok, 3, 0, 3), "NULL"),
        "d_q at 2^40": (([5, 6, 1 << 40, 8, 9], h_q, 5, *ok, 3, 0, 3), "2^40"),
        "h_q at -2^40": ((d_q, [1, 2, 3, -(1 << 40)], 5, *ok, 3, 0, 3), "2^40"),
        "device below -1": ((d_q, h_q, 5, *ok, 3, 0, 3, 2, 0, 0, -2), "device"),
        # the order: dispersion_call_args, the set table, the range, the depths
        "universe before permutations": ((d_q[:2], h_q[:1], 2, bad_pos, ok[1], 3, 0, 4, -1), "universe"),
        "permutations before the set table": ((d_q, h_q, 5, bad_pos, ok[1], 3, 0, 4, -1), "permutations"),
        "the set table before the range": ((d_q, h_q, 5, bad_pos, ok[1], 3, 0, 4), "outside the universe"),
        "the range before the depths": (([5, 6, 1 << 40, 8, 9], h_q, 5, *ok, 3, 0, 4), "triangle"),
        "the depths before the device": (([5, 6, 1 << 40, 8, 9], h_q, 5, *ok, 3, 0, 3, 2, 0, 0, -2), "2^40"),
    }
    for what, (args, word) in cases.items():
        assert _raw(*args) == _capi.ST_ERR_ARG, what
        assert word in _capi.last_error(), (what, _capi.last_error())
    # the tree entry refuses its own arguments before it looks at the tree
    L, p, c = _capi.load(), _capi._ptr, _capi.ctypes
    pos, off, univ = np.array(ok[0], dtype=np.int32), np.array(ok[1], dtype=np.int64), np.arange(5, dtype=np.int64)
    pd_q, union_q, bad, used = np.zeros(9, dtype=np.int64), np.zeros(9, dtype=np.int64), c.c_int64(0), c.c_int32(0)

    def tree_call(n=5, u=univ, begin=0, count=3, shift=-1, perms=2, stream=0, chunk=0):
        return L.st_unifrac_null_host(None, 0, p(u), n, p(pos), 6, p(off), 3, begin, count, shift, perms, 5, stream, chunk, p(pd_q), p(union_q),
                                      c.byref(used), c.byref(bad))
    for kw in ({"n": 2}, {"u": None}, {"count": 4}, {"shift": -2}, {"shift": 257}, {"chunk": -1}, {"perms": -1}, {"stream": -1}, {}):
        assert tree_call(**kw) == _capi.ST_ERR_ARG, kw
    assert "tree is NULL" in _capi.last_error()
    with pytest.raises(ValueError):
        _capi.unifrac_null_depths(d_q, h_q, [[0, 7]])
    with pytest.raises(ValueError):
        _capi.unifrac_null_depths(d_q, h_q[:3], [[0, 1]])
    with pytest.raises(ValueError):
        _capi.unifrac_null_depths(d_q, h_q, [[1, 0]])      # the library's own check: not increasing
    with pytest.raises(ValueError):
        _capi.unifrac_null_depths(d_q, h_q, [[0], [1]], begin=1, count=1)
    with pytest.raises(ValueError):
        _capi.unifrac_null_depths(d_q, h_q, [[0], [1]], permutations=-1)


def test_header_declares_and_capi_binds_the_exports():
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    L = _capi.load()
    for name in ("st_unifrac_null_host", "st_unifrac_null_depths"):
        assert ("int %s(" % name) in header and name in _capi.SYMBOLS and getattr(L, name).argtypes
    # additive exports: the ABI version stays where the other families' tests pin it
    assert "#define ST_API_VERSION %d\n" % _capi.API_VERSION in header and L.st_api_version() == _capi.API_VERSION


def test_facade_errors_raised_before_any_upload():
    import pandas as pd
    from suchtree_amd import SuchLinkedTrees, SuchTree, synth
    from suchtree_amd.exceptions import InvalidNodeError, NodeNotFoundError
    ta = SuchTree(synth.random_binary_tree(6, seed=1) + (["a%d" % i for i in range(6)],))
    tb = SuchTree(synth.random_binary_tree(9, seed=2) + (["b%d" % i for i in range(9)],))
    m = np.zeros((6, 9), dtype=int)
    m[0, :4] = m[1, 3:6] = m[2, 8] = 1
    slt = SuchLinkedTrees(ta, tb, pd.DataFrame(m, index=list(ta.leaves.keys()), columns=list(tb.leaves.keys())))
    for kw in ({"of": "C"}, {"pool": "all"}, {"min_partners": -1}, {"max_partners": 1.5}, {"begin": -1}, {"count": -1}, {"count": 4},
               {"begin": 2, "count": 2}, {"shift": -1}, {"shift": 2.5}, {"begin": True}, {"permutations": -1}, {"permutations": 2.5}, {"seed": -1}):
        with pytest.raises(ValueError):
            slt.partner_unifrac_null(**kw)
    names = list(tb.leaves.keys())
    inner = next(v for v in range(tb.size) if tb._flat.left[v] != -1 and v != tb.root_node and tb._flat.left[tb._flat.left[v]] != -1)
    for kw in ({"sets": [[names[0], names[0]]]},                              # a repeated member
               {"sets": [names], "root": inner},                               # a member that does not lie under root
               {"sets": [[names[0]]], "universe": names[1:]},                  # a member outside the universe
               {"sets": [[names[0]]], "universe": names[:2]},                  # a universe of two leaves
               {"sets": [[tb.root_node, tb.leaves[names[0]]]]},               # an id that is no leaf
               {"sets": [[names[0]]], "chunk_tasks": -1}, {"sets": [[names[0]]], "stream": -1},
               {"sets": [[names[0]], [names[1]]], "begin": 2}):
        with pytest.raises(ValueError):
            tb.unifrac_null(**kw)
    with pytest.raises(NodeNotFoundError):
        tb.unifrac_null([["nobody"]])
    with pytest.raises(InvalidNodeError):
        tb.unifrac_null([[names[0]]], root=tb.size)
    # no row: nothing is launched, and neither tree goes to a device
    none = slt.partner_unifrac_null(of="A", min_partners=5, permutations=3, seed=1)
    assert len(none) == 0 and none.count == 0 and len(none.leaves) == 0 and none.names == [] and none.root == tb.root_node
    assert none.permutations == 3 and none.seed == 1 and none.n_universe == 9
    assert ta._dev_tree is None and tb._dev_tree is None


def test_set_unifrac_null_on_a_hand_made_block():
    # a universe of 4; sets: 0 = the whole universe, 1 = the whole universe, 2 = two members, 3 = empty, 4 = one member
    perms, shift = 4, 1
    res = compare.SetUniFracNull(5, 0, 10, shift, perms, 7, 4, keep_null=True)
    pd_block = np.array([[40, 40, 40, 40, 40], [40, 40, 40, 40, 40], [20, 10, 20, 30, 26], [0, 0, 0, 0, 0], [8, 8, 6, 8, 12]], dtype=np.int64)
    res.fill_sets([4, 4, 2, 0, 1], pd_block)
    assert res.quantum == 0.5 and res.pd.tolist() == [20.0, 20.0, 10.0, 0.0, 4.0] and res.pd_q.tolist() == [40, 40, 20, 0, 8]
    # the whole-universe rule: the observation is the null
    for r in (0, 1):
        assert (res.pd_null_mean[r], res.pd_null_sd[r], res.pd_n_le[r], res.pd_n_ge[r], res.pd_p_le[r], res.pd_p_ge[r]) == (20.0, 0.0, 4, 4, 1.0, 1.0)
        assert np.isnan(res.pd_ses[r])
    # both tails of set 2: draws 5, 10, 15, 13 against 10
    draws = np.array([5.0, 10.0, 15.0, 13.0])
    assert res.null_pd[2].tolist() == draws.tolist()
    assert res.pd_null_mean[2] == draws.mean() and res.pd_null_sd[2] == draws.std(ddof=1)
    assert res.pd_ses[2] == (10.0 - draws.mean()) / draws.std(ddof=1)
    assert (res.pd_n_le[2], res.pd_n_ge[2], res.pd_p_le[2], res.pd_p_ge[2]) == (2, 3, 3 / 5, 4 / 5)
    # an empty set: every draw is 0, sd 0 exactly, SES NaN
    assert (res.pd_null_mean[3], res.pd_null_sd[3], res.pd_n_le[3], res.pd_n_ge[3]) == (0.0, 0.0, 4, 4) and np.isnan(res.pd_ses[3])
    # pairs in triangle order: (1,0) (2,0) (2,1) (3,0) (3,1) (3,2) (4,0) (4,1) (4,2) (4,3)
    union = np.zeros((10, perms + 1), dtype=np.int64)
    union[0] = 40                                   # two whole universes
    union[1] = union[2] = 40                        # a set inside the universe: the union is the universe
    union[3] = union[4] = 40                        # the empty set with the universe
    union[5] = pd_block[2]                          # the empty set with set 2: the union is set 2
    union[6] = union[7] = 40
    union[8] = [24, 18, 26, 30, 38]                 # sets 2 and 4: the draws differ
    union[9] = pd_block[4]
    res.fill_pairs(0, union[:4])
    res.fill_pairs(4, union[4:])                    # (two groups)
    assert res.union_q.tolist() == union[:, 0].tolist() and [res.pair(k) for k in (0, 5, 9)] == [(1, 0), (3, 2), (4, 3)]
    # pair 0: both whole -> the observation is the null, whatever the draws
    assert (res.unifrac[0], res.unifrac_null_mean[0], res.unifrac_null_sd[0], res.unifrac_n_le[0], res.unifrac_n_ge[0]) == (0.0, 0.0, 0.0, 4, 4)
    assert res.unifrac_p_le[0] == res.unifrac_p_ge[0] == 1.0 and np.isnan(res.unifrac_ses[0]) and res.phylosor[0] == 1.0
    # pair 8 by hand, from the integers by the expressions of SetUniFrac
    both = pd_block[2] + pd_block[4]
    uf = (2 * union[8] - both) / union[8]
    ps = 2 * (both - union[8]) / both
    assert res.unifrac[8] == uf[0] and res.null_unifrac[8].tolist() == uf[1:].tolist() and res.null_phylosor[8].tolist() == ps[1:].tolist()
    assert res.unifrac_null_mean[8] == pytest.approx(uf[1:].mean(), rel=1e-15) and res.unifrac_null_sd[8] == pytest.approx(uf[1:].std(ddof=1), rel=1e-14)
    assert res.unifrac_ses[8] == pytest.approx((uf[0] - uf[1:].mean()) / uf[1:].std(ddof=1), rel=1e-13)
    assert (res.unifrac_n_le[8], res.unifrac_n_ge[8]) == (int((uf[1:] <= uf[0]).sum()), int((uf[1:] >= uf[0]).sum()))
    assert res.unifrac_p_le[8] == (res.unifrac_n_le[8] + 1) / 5 and res.unifrac_p_ge[8] == (res.unifrac_n_ge[8] + 1) / 5
    assert res.phylosor_p_le[8] == (int((ps[1:] <= ps[0]).sum()) + 1) / 5 and res.n_nan[8] == 0
    # NaN draws where a union is empty: the empty set with a set whose PD draws hold a 0 ... (pair 9: set 4 and the empty set)
    zero = compare.SetUniFracNull(2, 0, 1, 0, 3, 1, 5, keep_null=True)
    zero.fill_sets([1, 0], np.array([[0, 0, 7, 9], [0, 0, 0, 0]], dtype=np.int64))      # a leaf at depth 0 in two columns
    zero.fill_pairs(0, np.array([[0, 0, 7, 9]], dtype=np.int64))
    assert np.isnan(zero.unifrac[0]) and np.isnan(zero.phylosor[0]) and zero.n_nan[0] == 1
    assert np.isnan(zero.null_unifrac[0, 0]) and zero.null_unifrac[0, 1:].tolist() == [1.0, 1.0] and zero.null_phylosor[0, 1:].tolist() == [0.0, 0.0]
    assert np.isnan(zero.unifrac_p_le[0]) and np.isnan(zero.unifrac_ses[0]) and zero.unifrac_null_mean[0] == 1.0 and zero.unifrac_null_sd[0] == 0.0
    # the rest of the interface
    assert len(res) == 5 and res.row(8)["i"] == 4 and res.row(8)["j"] == 2 and res.set_row(2)["pd_q"] == 20
    M = res.matrix("unifrac")
    assert M.shape == (5, 5) and M[4, 2] == M[2, 4] == res.unifrac[8] and not M.diagonal().any()
    with pytest.raises(ValueError):
        res.matrix("union_q")
    with pytest.raises(ValueError):
        compare.SetUniFracNull(5, 2, 3, 0, 1, 1, 4).matrix("unifrac")
    with pytest.raises(IndexError):
        res.pair(10)
    assert list(res.to_dataframe().columns) == ["i", "j"] + list(compare.SetUniFracNull.COLUMNS) and len(res.to_dataframe("sets")) == 5
    plain = compare.SetUniFracNull(5, 0, 10, shift, perms, 7, 4)
    assert plain.null_pd is None and plain.null_unifrac is None and plain.null_phylosor is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_unifrac_null_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_unifrac_null")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_unifrac_null.cpp"), os.path.join(csrc, "unifrac_plan.cpp"),
                           os.path.join(csrc, "unifrac_null_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize unifrac null ok" in out.stdout
