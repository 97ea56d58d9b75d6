"""The kernels of the UniFrac null on the GPU: st_unifrac_null_depths(device = 0) against its host restatement (pinned in
tests/test_unifrac_null_host.py to a composition of calls that exist without the feature), integer for integer, at the
sizes where a form can go wrong: universes of 3, 64, 65, 130 and 2049 leaves (one, two, three and 33 bitmap words -- at
2049 one word past kPermSmallMax, the sort's large class) and one of 16384 (256 words: four passes of the wave); sets of
0, 1, 2, 3, 32, 33, 64, 65, 256, 257 members and the whole universe; 70 permutations and 91 or 120 pairs, so that a wave of
64 pair tasks crosses from one row to the next and the last wave is partial.  Then the lane / wave threshold, more heavy tasks in a
chunk than the wave kernel's grid has waves, chunks and permutation blocks, either output alone, a range from mid-row to
mid-row, the tree path with an internal root, and the facade on gopher / louse.  Every comparison of integers is exact."""
import numpy as np
import pandas as pd
import pytest

import unifrac_null_reference as ref
from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 32, 33, 64, 65, 256, 257)
PERMS, SEED, STREAM = 70, 2024, 9


@pytest.fixture(scope="module")
def cases():
    """(d, h, sets, the host restatement's (pd_q, union_q) at 70 permutations) per universe size: computed once, never
    changed."""
    out = {}
    for n in (3, 64, 65, 130, 2049):
        d, h = ref.depths(n, n)
        sets = ref.sized_sets(n, SIZES, n + 1)
        out[n] = (d, h, sets, _capi.unifrac_null_depths(d, h, sets, permutations=PERMS, seed=SEED, stream=STREAM))
    return out


def _same(got, want, what):
    for name, g, w in (("pd_q", got[0], want[0]), ("union_q", got[1], want[1])):
        if g is None and w is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %d of %d %s differ, first at (row, p) %s: got %d want %d" % (what, len(bad), w.size, name, bad[0], g[tuple(bad[0])],
                                                                                               w[tuple(bad[0])])


def _device(d, h, sets, perms=PERMS, **kw):
    return _capi.unifrac_null_depths(d, h, sets, permutations=perms, seed=SEED, stream=STREAM, device=0, **kw)


@pytest.mark.parametrize("n", [3, 64, 65, 130, 2049])
def test_kernels_equal_the_restatement(cases, n):
    d, h, sets, want = cases[n]
    assert {len(s) for s in sets} >= {k for k in SIZES if k <= n} | {n}
    if n == 2049:      # both pair forms are at work, and the draws differ from the observation
        sizes = [len(s) for s in sets]
        assert max(sizes) * 2 > _capi.UNIFRAC_LANE_MAX and any(a + b <= _capi.UNIFRAC_LANE_MAX for a in sizes for b in sizes)
        assert (want[1][:, 1:] != want[1][:, :1]).any() and (want[0][:, 1:] != want[0][:, :1]).any()
    _same(_device(d, h, sets), want, "n %d" % n)
    # column 0 is the call without a null, on the device as on the host
    pd0, union0 = _capi.unifrac_depths(d, h, sets, device=0)
    assert (want[0][:, 0] == pd0).all() and (want[1][:, 0] == union0).all()


def test_the_largest_universe():
    n = _capi.HOMMOLA_MAX_UNIVERSE
    d, h = ref.depths(n, 5)
    rng = np.random.default_rng(6)
    sets = [np.arange(n), np.sort(rng.choice(n, 257, replace=False)), np.sort(rng.choice(n, 9000, replace=False)), np.array([0, n - 1])]
    want = _capi.unifrac_null_depths(d, h, sets, permutations=2, seed=SEED, stream=STREAM)
    _same(_device(d, h, sets, 2), want, "n 16384")
    assert (want[0][1, 1:] != want[0][1, 0]).all()


def test_lane_and_wave_forms_give_the_same_integers(cases, monkeypatch):
    for n in (130, 2049):
        d, h, sets, want = cases[n]
        for lane_max in ("0", "8", ""):
            monkeypatch.setenv("SUCHTREE_AMD_UNIFRAC_LANE_MAX", lane_max)
            _same(_device(d, h, sets), want, "n %d, lane_max %r" % (n, lane_max))


def test_more_heavy_tasks_in_a_chunk_than_the_wave_grid_has_waves(monkeypatch):
    """With the threshold at 0 every pair task is heavy.  14 sets and 100 permutations: 1414 set tasks, then 9191 pair tasks;
    chunks of 10000 tasks put 8586 pair tasks into the first, 85 whole pairs of them in one launch: 8585 heavy tasks, more
    than the 8192 waves of the wave kernel's grid, so its first waves take a second task.  The 86th pair's first row ends
    the chunk and its other rows begin the next: launches of one pair."""
    n, waves = 65, 2048 * 4      # unifrac_plan.h: kUnifracWaveBlocks workgroups of kUnifracThreads / 64 waves
    d, h = ref.depths(n, 21)
    sets = ref.sized_sets(n, (1, 2, 3, 5, 8, 13, 21, 32, 33, 64, 65), 22)
    assert len(sets) == 14 and 10000 - 14 * 101 > waves
    want = _capi.unifrac_null_depths(d, h, sets, permutations=100, seed=SEED, stream=STREAM)
    monkeypatch.setenv("SUCHTREE_AMD_UNIFRAC_LANE_MAX", "0")
    _same(_device(d, h, sets, 100, chunk_tasks=10000), want, "8585 heavy tasks in a launch")


def test_chunks_blocks_outputs_and_ranges(cases):
    d, h, sets, want = cases[130]
    total = len(want[1])
    # chunk_tasks bounds a chunk's tasks and a block's permutations: 64 makes two blocks of the 71 columns (64 and 7), 1 and
    # 3 make 71 and 24; chunks straddle the set tasks and the pair tasks of a block
    for chunk in (1, 3, 64, 0):
        _same(_device(d, h, sets, chunk_tasks=chunk), want, "chunk_tasks %d" % chunk)
    # either output alone: the other is not computed (the set tasks still write the table for the pairs)
    for chunk in (0, 64):
        _same(_device(d, h, sets, chunk_tasks=chunk, union=False), (want[0], None), "PD only, chunk_tasks %d" % chunk)
        _same(_device(d, h, sets, chunk_tasks=chunk, pd=False), (None, want[1]), "unions only, chunk_tasks %d" % chunk)
    # from inside row 4 to inside the last row
    begin, count = 4 * 3 // 2 + 2, total - 5 - (4 * 3 // 2 + 2)
    for chunk in (0, 50):
        got = _device(d, h, sets, begin=begin, count=count, chunk_tasks=chunk)
        _same(got, (want[0], want[1][begin:begin + count]), "a range from mid-row to mid-row, chunk_tasks %d" % chunk)
    # fewer permutations: a prefix; none: the observation; no pairs, no sets: nothing launched
    _same(_device(d, h, sets, 5), (want[0][:, :6], want[1][:, :6]), "5 permutations")
    _same(_device(d, h, sets, 0), (want[0][:, :1], want[1][:, :1]), "no permutation")
    assert _device(d, h, sets, begin=total, count=0)[1].shape == (0, PERMS + 1)
    assert _device(d, h, [])[0].shape == (0, PERMS + 1)


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links), links


def test_tree_path_with_an_internal_root():
    slt, _ = _slt("fish_worm")
    tb = slt.TreeB
    order = tb._depth_first_leaves()
    leaves = _capi.clade_plan(tb._flat.parent, np.sort(order))
    root = max((v for v in range(tb.size) if v != tb.root_node and tb._flat.left[v] != -1), key=lambda v: leaves["count"][v])
    lo, n = int(leaves["begin"][root]), int(leaves["count"][root])
    univ = order[lo:lo + n]
    assert 8 <= n < len(order)
    rng = np.random.default_rng(4)
    sets = [np.sort(rng.choice(n, int(k), replace=False)) for k in rng.integers(0, min(n, 40), 12)] + [np.arange(n), np.array([0, n - 1])]
    dev = tb._device_tree()
    perms, seed, stream = 6, 31, 5
    pd_q, union_q, shift = dev.unifrac_null_host(root, univ, sets, permutations=perms, seed=seed, stream=stream)
    # every column: the depths of the existing call, quantised, through the composition
    _, _, shift0, d, h = dev.unifrac_host(root, univ, sets)
    assert shift0 == shift
    d_q, h_q, _ = _capi.unifrac_quantise(d, h, shift)
    _same((pd_q, union_q), ref.compose(d_q, h_q, sets, perms, seed, stream), "tree path")
    # column 0 is SuchTree.unifrac at the shift reported: its universe is the members alone, this one every leaf under root,
    # and the range minimum over the wider universe is the depth of the same MRCA node
    direct = tb.unifrac([univ[s] for s in sets], root=root, shift=shift)
    assert (direct.pd_q == pd_q[:, 0]).all() and (direct.union_q == union_q[:, 0]).all()
    for chunk in (1, 7):
        again = dev.unifrac_null_host(root, univ, sets, 3, 40, None, perms, seed, stream, chunk_tasks=chunk)
        _same(again[:2], (pd_q, union_q[3:43]), "tree path, chunk_tasks %d" % chunk)
        assert again[2] == shift
    fixed = dev.unifrac_null_host(root, univ, sets, shift=shift - 3, permutations=2, seed=seed, stream=stream)
    d_q3, h_q3, _ = _capi.unifrac_quantise(d, h, shift - 3)
    _same(fixed[:2], ref.compose(d_q3, h_q3, sets, 2, seed, stream), "tree path, a caller's shift")
    with pytest.raises(ValueError):
        dev.unifrac_null_host(root, univ, sets, shift=shift + 1)      # the largest depth would reach 2^40
    for bad_univ, bad_root in ((np.append(univ[:-1], tb.size), root), (univ, tb.size)):
        with pytest.raises(_capi.InvalidNodeError):      # checked on the host, before anything is launched
            dev.unifrac_null_host(bad_root, bad_univ, sets)


def _state(slt):
    return (slt.subset_a_root, slt.subset_b_root, slt.subset_a_size, slt.subset_b_size, slt.subset_a_leafs.tolist(), slt.subset_b_leafs.tolist(),
            slt.subset_rows.tolist(), slt.subset_columns.tolist(), slt.linklist.tolist(), slt._seed)


def _check_against_composition(res, partner, root, universe, sets_ids, perms, seed):
    """``res`` (keep_null=True) against the composition over the universe ``universe`` (leaf ids) of the partner tree, the
    sets as leaf ids, sigma from hommola_permutation with stream = the partner tree's subset root."""
    order = partner._depth_first_leaves()
    inside = np.zeros(partner.size, dtype=bool)
    inside[universe] = True
    univ = order[inside[order]]
    n = len(univ)
    where = np.full(partner.size, -1, dtype=np.int64)
    where[univ] = np.arange(n)
    sets = [np.sort(where[np.asarray(ids, dtype=np.int64)]) for ids in sets_ids]
    assert all((s >= 0).all() for s in sets) and res.n_universe == n
    _, _, _, d, h = partner._device_tree().unifrac_host(root, univ, sets)
    d_q, h_q, _ = _capi.unifrac_quantise(d, h, res.shift)
    want_pd, want_union = ref.compose(d_q, h_q, sets, perms, seed, root, res.begin, res.count)
    assert (res.pd_q == want_pd[:, 0]).all() and (res.union_q == want_union[:, 0]).all()
    assert res.null_pd.tobytes() == (want_pd[:, 1:].astype(np.float64) * res.quantum).tobytes()
    i, j = compare.SetUniFrac._rows(res.begin + np.arange(res.count, dtype=np.int64))
    both = want_pd[i] + want_pd[j]
    with np.errstate(invalid="ignore", divide="ignore"):
        unifrac = np.where(want_union != 0, (2 * want_union - both) / want_union.astype(np.float64), np.nan)
        phylosor = np.where(both != 0, 2 * (both - want_union) / both.astype(np.float64), np.nan)
    for name, x in (("unifrac", unifrac), ("phylosor", phylosor)):
        assert np.array_equal(getattr(res, name), x[:, 0], equal_nan=True) and np.array_equal(getattr(res, "null_" + name), x[:, 1:], equal_nan=True)
        whole = (res.n[i] == n) & (res.n[j] == n)
        mean, sd, ses, n_le = compare.null_summary(x[:, 0], x[:, 1:], whole)
        for suffix, v in (("_null_mean", mean), ("_null_sd", sd), ("_ses", ses), ("_n_le", n_le)):
            assert np.array_equal(getattr(res, name + suffix), v, equal_nan=True), name + suffix
        n_ge = np.where(whole, perms, (x[:, 1:] >= x[:, :1]).sum(axis=1))
        assert (getattr(res, name + "_n_ge") == n_ge).all()
        assert np.array_equal(getattr(res, name + "_p_ge"), np.where(np.isnan(x[:, 0]), np.nan, (n_ge + 1) / (perms + 1)), equal_nan=True)
    return sets


@pytest.mark.parametrize("of", ["A", "B"])
def test_partner_unifrac_null_on_gopher_louse(of):
    slt, links = _slt("gopher_louse")
    before = _state(slt)
    perms, seed = 9, 3
    res = slt.partner_unifrac_null(of=of, permutations=perms, seed=seed, keep_null=True)
    assert _state(slt) == before
    own, partner = (slt.TreeA, slt.TreeB) if of == "A" else (slt.TreeB, slt.TreeA)
    plain = slt.partner_unifrac(of=of, shift=res.shift)
    assert res.names == plain.names and res.leaves.tolist() == plain.leaves.tolist() and res.root == plain.root == partner.root_node
    assert (res.pd_q == plain.pd_q).all() and (res.union_q == plain.union_q).all()
    assert np.array_equal(res.unifrac, plain.unifrac, equal_nan=True) and np.array_equal(res.phylosor, plain.phylosor, equal_nan=True)
    assert res.permutations == perms and res.seed == seed and res.null_unifrac.shape == (res.count, perms) and res.n_universe == partner.num_leaves
    ll = slt.linklist
    own_col, partner_col = (1, 0) if of == "A" else (0, 1)
    sets_ids = [ll[ll[:, own_col] == leaf, partner_col] for leaf in res.leaves]
    root = int(slt.subset_b_root if of == "A" else slt.subset_a_root)
    _check_against_composition(res, partner, root, partner._depth_first_leaves(), sets_ids, perms, seed)
    # the same seed and pool relabel the sets exactly as partner_dispersion does: its universe, its rows, its stream
    disp = slt.partner_dispersion(of=of, permutations=perms, seed=seed, min_partners=1)
    assert disp.names == res.names and disp.n_universe == res.n_universe and disp.seed == res.seed
    # SuchTree.unifrac_null on the same sets by name, with the stream the facade passes
    names = partner.leaf_nodes
    direct = partner.unifrac_null([[names[int(b)] for b in ids] for ids in sets_ids], permutations=perms, seed=seed, stream=root, keep_null=True)
    assert direct.null_pd.tobytes() == res.null_pd.tobytes() and direct.null_unifrac.tobytes() == res.null_unifrac.tobytes()
    assert direct.shift == res.shift and direct.pd_ses.tobytes() == res.pd_ses.tobytes()
    # fewer permutations: a prefix of the draws; a range at the shift: the same columns
    short = slt.partner_unifrac_null(of=of, permutations=4, seed=seed, keep_null=True, begin=2, count=5, shift=res.shift)
    assert short.null_unifrac.tobytes() == np.ascontiguousarray(res.null_unifrac[2:7, :4]).tobytes()
    assert short.null_pd.tobytes() == np.ascontiguousarray(res.null_pd[:, :4]).tobytes() and short.pair(0) == res.pair(2)
    assert res.row(0)["name_i"] == res.names[1] and len(res.to_dataframe()) == res.count and len(res.to_dataframe("sets")) == len(res)


def test_partner_unifrac_null_under_a_subset_with_both_pools():
    slt, _ = _slt("gopher_louse")
    found = False
    for node in slt.TreeA.internal_nodes:      # under a subset of TreeA the linked pool is smaller than the partner tree's subset
        slt.subset_a(int(node))
        linked = np.unique(slt.linklist[:, 0])
        if 3 <= len(linked) < slt.subset_b_size and len(np.unique(slt.linklist[:, 1])) >= 3:
            found = True
            break
    assert found
    before = _state(slt)
    perms, seed = 7, 12
    ll = slt.linklist
    root = int(slt.subset_b_root)
    for pool, universe in (("subset", np.asarray(slt.subset_b_leafs, dtype=np.int64)), ("linked", linked)):
        res = slt.partner_unifrac_null(of="A", pool=pool, permutations=perms, seed=seed, keep_null=True)
        assert _state(slt) == before
        disp = slt.partner_dispersion(of="A", pool=pool, permutations=perms, seed=seed, min_partners=1)
        assert disp.names == res.names and disp.n_universe == res.n_universe == len(universe) and res.root == root
        sets_ids = [ll[ll[:, 1] == leaf, 0] for leaf in res.leaves]
        _check_against_composition(res, slt.TreeB, root, universe, sets_ids, perms, seed)
