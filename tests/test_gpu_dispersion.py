"""The partner-dispersion kernels on the GPU: st_dispersion_matrix(device = 0) against its host restatement bit for bit
over the size-class edges (the packed class of 6 .. 30 positions among them), universes on both sides of every sort's
limit up to 8193 positions (more than 128 KiB of sort keys), the tree path (st_partner_dispersion_host) on fish_worm, and the facade
(SuchTree.dispersion, SuchLinkedTrees.partner_dispersion).  The bounds are those of tests/test_dispersion_host.py:
relative k^2 2^-52 for MPD and k 2^-52 for MNTD."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, n)) * 10.0 ** rng.integers(-2, 2, (n, n))).astype(np.float32)


def _sets(n, sizes, seed):
    """One set per size that fits, then a set nested in the largest one, the largest again and the first again."""
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in sizes if k <= n]
    big = max(sets, key=len)
    return sets + [big[: max(2, len(big) // 2)], big.copy(), sets[0].copy(), np.arange(n)]


@pytest.fixture(scope="module")
def cases():
    """(D, sets, the host restatement's records at 17 permutations) per universe size: computed once, never changed."""
    out = {}
    for n in (3, 64, 65, 129, 2048, 2049):
        D, sets = _matrix(n, n), _sets(n, SIZES, n + 1)
        out[n] = (D, sets, _capi.dispersion_matrix(D, sets, 17, 4242 + n, stream=6, device=-1))
    return out


@pytest.mark.parametrize("perms", [0, 1, 17])
@pytest.mark.parametrize("n", [3, 64, 65, 129, 2048, 2049])
def test_kernels_equal_the_restatement(cases, n, perms):
    D, sets, want = cases[n]
    want = np.ascontiguousarray(want[:, : perms + 1])      # (the prefix property of the restatement: test_dispersion_host.py)
    for chunk in (0, 1, 7):
        got = _capi.dispersion_matrix(D, sets, perms, 4242 + n, stream=6, device=0, chunk_tasks=chunk)
        bad = np.argwhere((got["pair_sum"].view(np.int64) != want["pair_sum"].view(np.int64))
                          | (got["nearest_sum"].view(np.int64) != want["nearest_sum"].view(np.int64)))
        assert len(bad) == 0, ("chunk_tasks %d: %d records differ, first (set, p) %s of size %d: got %s want %s"
                               % (chunk, len(bad), bad[0], len(sets[bad[0][0]]), got[tuple(bad[0])], want[tuple(bad[0])]))
    assert want[-3].tobytes() == want[len([k for k in SIZES if k <= n]) - 1].tobytes()      # identical sets, identical bits


def test_special_values_and_large_universe():
    """A universe whose sort needs more than 32 KiB of LDS (1024 lanes), a set that is the whole universe, and the
    comparison rule on NaN, +inf and -0.0 entries."""
    n = 4097
    D = _matrix(n, 9)
    rng = np.random.default_rng(10)
    D[rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = np.nan
    D[rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = np.inf
    D[rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = -0.0
    D[rng.integers(0, n, 2000), rng.integers(0, n, 2000)] = 0.0
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in (2, 5, 64, 65, 513)] + [np.arange(n)]
    want = _capi.dispersion_matrix(D, sets, 1, 5, device=-1)
    got = _capi.dispersion_matrix(D, sets, 1, 5, device=0)
    assert got.tobytes() == want.tobytes()
    assert np.isnan(want["pair_sum"][-1]).all() and np.isfinite(want["nearest_sum"][-1]).all()      # NaN entries: summed, never a minimum


def test_universe_above_8192_positions():
    """8193 positions: k_dispersion_sigma<1024> with more than 8 keys per lane (128 KiB of sort keys and more)."""
    n = 8193
    i = np.arange(n, dtype=np.int32)
    D = ((i[:, None] * 31 + i[None, :] * 17) % 1009).astype(np.float32)
    rng = np.random.default_rng(8193)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in (2, 16, 65, 300)]
    want = _capi.dispersion_matrix(D, sets, 2, 8193, stream=3, device=-1)
    assert want.shape == (4, 3)
    for chunk in (0, 3):
        got = _capi.dispersion_matrix(D, sets, 2, 8193, stream=3, device=0, chunk_tasks=chunk)
        assert got.tobytes() == want.tobytes(), "chunk_tasks %d" % chunk
    assert want[:, 1].tobytes() != want[:, 0].tobytes() and want[:, 2].tobytes() != want[:, 1].tobytes()      # the draws differ


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links), links


def test_tree_path_on_fish_worm():
    slt, links = _slt("fish_worm")
    tb = slt.TreeB
    univ = tb._depth_first_leaves()
    n = len(univ)
    where = np.full(tb.size, -1, dtype=np.int64)
    where[univ] = np.arange(n)
    ll = slt.linklist
    fish = [f for f in np.unique(ll[:, 1]) if np.count_nonzero(ll[:, 1] == f) >= 2]
    sets = [np.sort(where[ll[ll[:, 1] == f, 0]]) for f in fish]
    dev = tb._device_tree()
    perms, seed, stream = 9, 11, int(tb.root_node)
    got = dev.partner_dispersion_host(univ, sets, perms, seed, stream)
    # the float32 matrix of the existing grid path: D[a][b] = dist(u[a], u[b])
    D = dev.grid_host(univ, univ)[0].reshape(n, n).astype(np.float32)
    want = _capi.dispersion_matrix(D, sets, perms, seed, stream=stream, device=-1)
    assert got.tobytes() == want.tobytes()
    for chunk in (1, 7):
        assert dev.partner_dispersion_host(univ, sets, perms, seed, stream, chunk_tasks=chunk).tobytes() == want.tobytes()
    # Row p = 0 against float64 numpy over pairwise_distances.  The bounds cover the order of the float64 adds, so both
    # sides must add the same float32 values: D[a][b] = dist(u[a], u[b]) keeps both triangles, and pairwise_distances
    # evaluates entry [i, j], i < j, as d(ids[i], ids[j]) and mirrors it.  The lower triangle therefore comes from the
    # upper triangle of a second call over the reversed list.  (Against the mirrored matrix of one call MPD is off by
    # up to 3.6e-8 relative on these fish -- the last bit of a float32 distance, which depends on the argument order --
    # against bounds of 1e-15 .. 5e-13.)
    ids = univ.tolist()
    M = np.triu(tb.pairwise_distances(ids)) + np.tril(tb.pairwise_distances(ids[::-1])[::-1, ::-1])
    for r, s in enumerate(sets):
        k = len(s)
        sub = M[np.ix_(s, s)]
        off = sub[~np.eye(k, dtype=bool)].reshape(k, k - 1)
        want_mpd, want_mntd = off.sum() / (k * (k - 1)), off.min(axis=1).sum() / k
        mpd, mntd = got[r, 0]["pair_sum"] / (k * (k - 1)), got[r, 0]["nearest_sum"] / k
        print("fish %d, k %d: mpd rel err %.3g (bound %.3g), mntd rel err %.3g (bound %.3g)"
              % (fish[r], k, abs(mpd - want_mpd) / want_mpd, k * k * 2.0 ** -52, abs(mntd - want_mntd) / want_mntd, k * 2.0 ** -52))
        assert abs(mpd - want_mpd) <= k * k * 2.0 ** -52 * want_mpd
        assert abs(mntd - want_mntd) <= k * 2.0 ** -52 * want_mntd
    with pytest.raises(_capi.InvalidNodeError):
        dev.partner_dispersion_host(np.append(univ[:-1], tb.size), sets, perms, seed, stream)


def _state(slt):
    return (slt.subset_a_root, slt.subset_b_root, slt.subset_a_size, slt.subset_b_size, slt.subset_a_leafs.tolist(), slt.subset_b_leafs.tolist(),
            slt.subset_rows.tolist(), slt.subset_columns.tolist(), slt.linklist.tolist(), slt._seed)


def test_facade_fish_worm():
    slt, links = _slt("fish_worm")
    before = _state(slt)
    res = slt.partner_dispersion(of="A", permutations=99, seed=3, min_partners=3, keep_null=True)
    assert _state(slt) == before
    counts = (links > 0).sum(axis=1)
    assert len(res) == 19 == int((counts >= 3).sum())
    assert sorted(res.names) == sorted(counts.index[counts >= 3]) and res.n.tolist() == [int(counts[name]) for name in res.names]
    assert res.leaves.tolist() == [slt.TreeA.leaves[name] for name in res.names] and res.n_universe == slt.TreeB.num_leaves
    assert res.permutations == 99 and res.seed == 3 and res.null_mpd.shape == (19, 99)
    # one row by hand: the partners' distances from pairwise_distances, the null from the kept draws
    i = int(np.argmax(res.n))
    partners = slt.linklist[slt.linklist[:, 1] == res.leaves[i], 0]
    M = slt.TreeB.pairwise_distances(partners.tolist())
    k = len(partners)
    off = M[~np.eye(k, dtype=bool)].reshape(k, k - 1)
    assert abs(res.mpd[i] - off.mean()) < 1e-6 * off.mean() and abs(res.mntd[i] - off.min(axis=1).mean()) < 1e-6 * off.mean()
    null = res.null_mpd[i]
    assert abs(res.mpd_null_mean[i] - null.mean()) < 1e-12 and abs(res.mpd_null_sd[i] - null.std(ddof=1)) < 1e-12
    assert abs(res.mpd_ses[i] - (res.mpd[i] - null.mean()) / null.std(ddof=1)) < 1e-9
    assert res.mpd_n_le[i] == np.count_nonzero(null <= res.mpd[i]) and res.mpd_p[i] == (res.mpd_n_le[i] + 1) / 100
    assert (res.n_nan == 0).all() and res.row(i)["name"] == res.names[i] and len(res.to_dataframe()) == 19
    # the same seed gives the same bits, and fewer permutations a prefix of the draws
    short = slt.partner_dispersion(of="A", permutations=5, seed=3, min_partners=3, keep_null=True)
    assert short.null_mntd.tobytes() == np.ascontiguousarray(res.null_mntd[:, :5]).tobytes() and short.mpd.tobytes() == res.mpd.tobytes()
    # the draws are SuchTree.dispersion's with stream = the partner tree's subset root
    names_b = slt.TreeB.leaf_nodes
    direct = slt.TreeB.dispersion([[names_b[int(b)] for b in partners]], permutations=5, seed=3, stream=int(slt.subset_b_root), keep_null=True)
    assert direct.null_mpd[0].tobytes() == short.null_mpd[i].tobytes()


def test_facade_mirror_launches_nothing():
    slt, links = _slt("fish_worm")
    res = slt.partner_dispersion(of="B", permutations=9, seed=1, min_partners=2)
    assert len(res) == 0 and res.names == [] and res.n_universe == slt.TreeA.num_leaves
    assert slt.TreeA._dev_tree is None and slt.TreeB._dev_tree is None      # nothing was uploaded, nothing launched


def test_facade_gopher_louse_and_pools():
    slt, links = _slt("gopher_louse")
    res = slt.partner_dispersion(of="A", permutations=19, seed=2)
    counts = (links > 0).sum(axis=1)
    two = sorted(counts.index[counts == 2])
    assert len(two) == 2 and sorted(name for name, k in zip(res.names, res.n) if k == 2) == two
    assert sorted(res.names) == sorted(counts.index[counts >= 2])
    # under a subset of TreeA the linked pool is smaller than the partner tree's subset
    found = False
    for node in slt.TreeA.internal_nodes:
        slt.subset_a(int(node))
        linked = len(np.unique(slt.linklist[:, 0]))
        if 3 <= linked < slt.subset_b_size and np.count_nonzero(np.bincount(slt.linklist[:, 1]) >= 2):
            found = True
            break
    assert found
    before = _state(slt)
    sub = slt.partner_dispersion(of="A", permutations=19, seed=2, pool="subset")
    lnk = slt.partner_dispersion(of="A", permutations=19, seed=2, pool="linked")
    assert _state(slt) == before
    assert sub.n_universe == slt.subset_b_size and lnk.n_universe == linked and sub.n_universe != lnk.n_universe
    assert sub.names == lnk.names and len(sub) > 0
    assert sub.mpd.tobytes() == lnk.mpd.tobytes() and sub.mntd.tobytes() == lnk.mntd.tobytes()      # the observation does not depend on the pool
    assert not np.array_equal(sub.mpd_null_mean, lnk.mpd_null_mean)
