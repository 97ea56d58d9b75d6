"""The between-set dispersion kernels on the GPU: st_beta_dispersion_matrix(device = 0) against its host restatement bit for
bit over the cross-product of lane-set sizes (1, 2, 3, 32, 33, 64, 65, 257: every form, both sides of each edge) and
walked-set sizes (1, 7, 8, 9, 64, 65, 513: the unroll edge, staging past one wave, several broadcast words), on nested and
overlapping sets, with and without exclude_shared; a range cut mid-row; the special values; the tree path
(st_beta_dispersion_host) on fish_worm; the facade on gopher_louse.

Bounds against tests/beta_dispersion_reference.py are those of tests/test_beta_dispersion_host.py: relative k_r k_c 2^-52
for a cross sum and k_r 2^-52 for a nearest sum.  beta_mpd and beta_mntd add two such sums and divide once, on both
sides of the comparison: two more roundings of 2^-53 each side, so (k_i k_j + 2) 2^-52 and (max(k_i, k_j) + 2) 2^-52."""
import numpy as np
import pandas as pd
import pytest

import beta_dispersion_reference as ref
from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu

LANE_SIZES = (1, 2, 3, 32, 33, 64, 65, 257)
WALK_SIZES = (1, 7, 8, 9, 64, 65, 513)


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, n)) * 10.0 ** rng.integers(-2, 2, (n, n))).astype(np.float32)


def _sets(n, seed):
    """One set per size of either list that fits, each a prefix of one shuffle of the universe (a nested chain); then sets
    that overlap them without being nested, a second set of one member equal to the first, and a third that differs: with
    every pair taken in both directions, every (k_r, k_c) of the two lists occurs, equal sizes included."""
    order = np.random.default_rng(seed).permutation(n)
    sizes = sorted(set(LANE_SIZES) | set(WALK_SIZES))
    sets = [np.sort(order[:k]) for k in sizes if k <= n]
    extra = [order[:1]] + [order[a:a + k] for a, k in ((1, 1), (32, 64), (30, 65)) if a + k <= n]
    return sets + [np.sort(s) for s in extra]


def _differences(got, want):
    return np.argwhere((got["pair_sum"].view(np.int64) != want["pair_sum"].view(np.int64))
                       | (got["nearest_sum"].view(np.int64) != want["nearest_sum"].view(np.int64)))


@pytest.fixture(scope="module")
def cases():
    """(D, sets, the host restatement's records at 17 permutations) per (universe size, exclude_shared): computed once,
    never changed."""
    out = {}
    for n in (3, 65, 2049):
        D, sets = _matrix(n, n), _sets(n, n + 1)
        for exclude in (False, True):
            out[n, exclude] = (D, sets, _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=17, seed=4242 + n, stream=6))
    return out


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("perms", [0, 1, 17])
@pytest.mark.parametrize("n", [3, 65, 2049])
def test_kernels_equal_the_restatement(cases, n, perms, exclude):
    D, sets, want = cases[n, exclude]
    if n == 2049:      # every combination of the two lists is there
        have = {(len(a), len(b)) for a in sets for b in sets if a is not b}
        assert all((kr, kc) in have for kr in LANE_SIZES for kc in WALK_SIZES)
    want = np.ascontiguousarray(want[:, :, : perms + 1])      # (the prefix property of the restatement: test_beta_dispersion_host.py)
    for chunk in (0, 1, 7):
        got = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=perms, seed=4242 + n, stream=6, device=0, chunk_tasks=chunk)
        bad = _differences(got, want)
        if len(bad):
            i, j = compare.SetUniFrac._rows(bad[:1, 0])
            r, c = (i[0], j[0]) if bad[0][1] == 0 else (j[0], i[0])
            assert False, ("chunk_tasks %d: %d records differ, first (pair, dir, p) %s, k_r %d, k_c %d: got %s want %s"
                           % (chunk, len(bad), bad[0], len(sets[r]), len(sets[c]), got[tuple(bad[0])], want[tuple(bad[0])]))


def test_range_cut_mid_row(cases):
    D, sets, want = cases[2049, True]
    total = len(want)
    begin, count = 4, total - 9      # starts inside row 3, ends inside the last row
    for chunk in (0, 5):
        got = _capi.beta_dispersion_matrix(D, sets, begin, count, True, 17, 4242 + 2049, 6, device=0, chunk_tasks=chunk)
        assert got.tobytes() == np.ascontiguousarray(want[begin:begin + count]).tobytes()
    assert _capi.beta_dispersion_matrix(D, sets, total, 0, True, 17, 1, 6, device=0).shape == (0, 2, 18)      # no pair: nothing launched


def test_special_values():
    """The comparison rule on NaN, +inf and -0.0 entries, in every form."""
    n = 600
    D = _matrix(n, 9)
    rng = np.random.default_rng(10)
    for value in (np.nan, np.inf, -0.0, 0.0):
        D[rng.integers(0, n, 3000), rng.integers(0, n, 3000)] = value
    sets = _sets(n, 11)
    for exclude in (False, True):
        want = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=1, seed=5)
        got = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=1, seed=5, device=0)
        assert got.tobytes() == want.tobytes()
    assert np.isnan(want["pair_sum"]).any() and np.isinf(want["nearest_sum"]).any() and not np.isnan(want["nearest_sum"]).any()


def test_walked_set_above_32_kib_of_lds():
    """A walked set of more than 8192 members with exclude_shared: the workgroup form stages more than 32 KiB (q' and the
    positions), which has to be asked for."""
    n = 8200
    i = np.arange(n, dtype=np.int32)
    D = ((i[:, None] * 31 + i[None, :] * 17) % 1009).astype(np.float32)
    rng = np.random.default_rng(n)
    sets = [np.arange(n), np.sort(rng.choice(n, 65, replace=False)), np.sort(rng.choice(n, 300, replace=False))]
    want = _capi.beta_dispersion_matrix(D, sets, exclude_shared=True, permutations=1, seed=n, stream=3)
    got = _capi.beta_dispersion_matrix(D, sets, exclude_shared=True, permutations=1, seed=n, stream=3, device=0)
    assert got.tobytes() == want.tobytes()
    assert want[:, :, 1].tobytes() != want[:, :, 0].tobytes()      # the draw differs from the observation


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links), links


def _within_bounds(D, sets, rec, seed, stream, exclude, begin=0):
    """Column p = 0 .. of ``rec`` against the reference module, within the bounds of the module docstring."""
    for p in range(rec.shape[2]):
        sigma = compare.hommola_permutation(seed, stream, p, 0, len(D))
        for k, (i, j) in enumerate(ref.pairs(len(sets), begin, rec.shape[0])):
            for d, (r, c) in enumerate(((i, j), (j, i))):
                cross, near, _ = ref.direction(D, sigma, sets[r], sets[c], exclude)
                kr, kc = len(sets[r]), len(sets[c])
                assert abs(rec[k, d, p]["pair_sum"] - cross) <= kr * kc * 2.0 ** -52 * cross, (i, j, d, p)
                assert abs(rec[k, d, p]["nearest_sum"] - near) <= kr * 2.0 ** -52 * near, (i, j, d, p)


def test_tree_path_on_fish_worm():
    slt, links = _slt("fish_worm")
    tb = slt.TreeB
    univ = tb._depth_first_leaves()
    n = len(univ)
    where = np.full(tb.size, -1, dtype=np.int64)
    where[univ] = np.arange(n)
    ll = slt.linklist
    sets = [np.sort(where[ll[ll[:, 1] == f, 0]]) for f in np.unique(ll[:, 1])][:8]
    sets = sets + [np.union1d(a, b) for a, b in zip(sets, sets[1:])]      # (a worm has one fish: unions make the sets overlap)
    dev = tb._device_tree()
    perms, seed, stream = 5, 11, int(tb.root_node)
    # the float32 matrix of the existing grid path: D[a][b] = dist(u[a], u[b])
    D = dev.grid_host(univ, univ)[0].reshape(n, n).astype(np.float32)
    for exclude in (False, True):
        got = dev.beta_dispersion_host(univ, sets, 0, None, exclude, perms, seed, stream)
        want = _capi.beta_dispersion_matrix(D, sets, exclude_shared=exclude, permutations=perms, seed=seed, stream=stream)
        assert got.tobytes() == want.tobytes()
        for chunk in (1, 7):
            assert dev.beta_dispersion_host(univ, sets, 3, 20, exclude, perms, seed, stream, chunk_tasks=chunk).tobytes() == want[3:23].tobytes()
        _within_bounds(D, sets, got[:, :, :2], seed, stream, exclude)
    with pytest.raises(_capi.InvalidNodeError):
        dev.beta_dispersion_host(np.append(univ[:-1], tb.size), sets, permutations=perms, seed=seed, stream=stream)


def _state(slt):
    return (slt.subset_a_root, slt.subset_b_root, slt.subset_a_size, slt.subset_b_size, slt.subset_a_leafs.tolist(), slt.subset_b_leafs.tolist(),
            slt.subset_rows.tolist(), slt.subset_columns.tolist(), slt.linklist.tolist(), slt._seed)


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("of", ["A", "B"])
def test_partner_beta_dispersion_on_gopher_louse(of, exclude):
    slt, links = _slt("gopher_louse")
    before = _state(slt)
    perms, seed = 9, 3
    res = slt.partner_beta_dispersion(of=of, exclude_shared=exclude, permutations=perms, seed=seed, keep_null=True)
    assert _state(slt) == before
    own, partner = (slt.TreeA, slt.TreeB) if of == "A" else (slt.TreeB, slt.TreeA)
    counts = (links > 0).sum(axis=1 if of == "A" else 0)
    assert sorted(res.names) == sorted(counts.index[counts >= 1]) and res.leaves.tolist() == [own.leaves[name] for name in res.names]
    assert res.n_sets == len(res.names) and len(res) == res.n_sets * (res.n_sets - 1) // 2 and res.n_universe == partner.num_leaves
    assert res.permutations == perms and res.seed == seed and res.null_beta_mntd.shape == (len(res), perms)
    # the sets and the matrix by hand: the partners of every row as positions of the partner tree's depth-first leaves
    univ = partner._depth_first_leaves()
    n = len(univ)
    where = np.full(partner.size, -1, dtype=np.int64)
    where[univ] = np.arange(n)
    ll = slt.linklist
    own_col, partner_col = (1, 0) if of == "A" else (0, 1)
    sets = [np.sort(where[ll[ll[:, own_col] == leaf, partner_col]]) for leaf in res.leaves]
    D = partner._device_tree().grid_host(univ, univ)[0].reshape(n, n).astype(np.float32)
    stream = int(slt.subset_b_root if of == "A" else slt.subset_a_root)
    sigmas = [compare.hommola_permutation(seed, stream, p, 0, n) for p in range(perms + 1)]
    assert (res.n_i > 1).any() if of == "A" else (res.shared > 0).any()      # (a gopher has up to two lice; two lice share a gopher)
    for at, (i, j) in enumerate(ref.pairs(len(sets))):
        ki, kj = len(sets[i]), len(sets[j])
        assert (res.n_i[at], res.n_j[at], res.shared[at]) == (ki, kj, len(np.intersect1d(sets[i], sets[j])))
        draws = np.array([ref.beta(D, s, sets[i], sets[j], exclude) for s in sigmas])
        for col, name, bound in ((0, "beta_mpd", (ki * kj + 2) * 2.0 ** -52), (1, "beta_mntd", (max(ki, kj) + 2) * 2.0 ** -52)):
            got = np.concatenate([[getattr(res, name)[at]], getattr(res, "null_" + name)[at]])
            both_nan = np.isnan(got) & np.isnan(draws[:, col])
            assert (both_nan | (np.abs(got - draws[:, col]) <= bound * draws[:, col])).all(), (i, j, name, got, draws[:, col])
            if not np.isnan(got[0]):
                want = ref.null_columns(got[0], got[1:])
                for suffix, v in want.items():
                    g = getattr(res, name + suffix)[at]
                    assert (np.isnan(v) and np.isnan(g)) or abs(g - v) <= 1e-9 * max(1.0, abs(v)), (i, j, name + suffix, g, v)
    assert res.row(0)["name_i"] == res.names[1] and res.row(0)["name_j"] == res.names[0] and len(res.to_dataframe()) == len(res)
    M = res.matrix("beta_mntd")
    assert M.shape == (res.n_sets, res.n_sets) and (np.isnan(res.beta_mntd[0]) or M[1, 0] == M[0, 1] == res.beta_mntd[0])
    # fewer permutations: a prefix of the draws; a range: the same columns
    short = slt.partner_beta_dispersion(of=of, exclude_shared=exclude, permutations=4, seed=seed, keep_null=True, begin=2, count=5)
    assert short.null_beta_mpd.tobytes() == np.ascontiguousarray(res.null_beta_mpd[2:7, :4]).tobytes()
    assert short.beta_mntd.tobytes() == res.beta_mntd[2:7].tobytes() and short.pair(0) == res.pair(2)
