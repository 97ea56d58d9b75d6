"""Hommola's permutation test on the GPU (SuchLinkedTrees.hommola_cospeciation, C ABI st_compare_rows_host): the fixtures
against a numpy restatement of scikit-bio's test on the oracle's distances, every row's bits independent of its position,
its batch and the chunk size, large rows against numpy float64, seeds, subsets, errors and NaN."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from oracle.oracle import OracleTree
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.compare import DistanceComparison, hommola_rows, row_stats, _SUMS
from suchtree_amd.linked import SuchLinkedTrees

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_moments(c, x, y):      # (the bars of tests/test_gpu_compare.py)
    assert c.n_pairs == len(x)
    for got, want in ((c.mean_x, x.mean()), (c.mean_y, y.mean()), (c.var_x, np.var(x)), (c.var_y, np.var(y)),
                      (c.cov, np.cov(x, y, bias=True)[0, 1])):
        assert _rel(got, want) < 1e-10, (got, want)
    dx, dy = x - c.shift_x, y - c.shift_y
    for got, want in ((c.sxx, (dx * dx).sum()), (c.syy, (dy * dy).sum()), (c.sxy, (dx * dy).sum())):
        assert _rel(got, want) < 1e-10, (got, want)
    assert abs(c.sx - dx.sum()) < 1e-10 * np.sqrt(len(x) * c.sxx) and abs(c.sy - dy.sum()) < 1e-10 * np.sqrt(len(y) * c.syy)
    assert (c.min_x, c.max_x, c.min_y, c.max_y) == (x.min(), x.max(), y.min(), y.max())
    assert abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-12


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


def _state(S):
    return (S.subset_a_root, S.subset_b_root, S.subset_a_size, S.subset_b_size, S.subset_n_links,
            S.subset_a_leafs.copy(), S.subset_b_leafs.copy(), S.linklist.copy())


def _same_state(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _universes(S):
    """(u_a, u_b, pos_a, pos_b) of the current subset: the universes and each link's positions in them."""
    u_a, u_b = np.asarray(S.subset_a_leafs, np.int64), np.asarray(S.subset_b_leafs, np.int64)
    ll = S.linklist
    pos_a = np.array([int(np.flatnonzero(u_a == v)[0]) for v in ll[:, 1]])
    pos_b = np.array([int(np.flatnonzero(u_b == v)[0]) for v in ll[:, 0]])
    return u_a, u_b, pos_a, pos_b


def _restated(S, permutations, seed):
    """scikit-bio's hommola_cospeciation in numpy: ordered distance matrices over the universes (the oracle's distances),
    the same draws, each relabelled row's pairs in the orientation of linked_distances(), float64 Pearson."""
    u_a, u_b, pos_a, pos_b = _universes(S)
    ll = S.linklist
    mats = []
    for T, u in ((S.TreeA, u_a), (S.TreeB, u_b)):
        O = OracleTree(T._flat.parent, T._flat.distance)
        i, j = np.meshgrid(np.arange(len(u)), np.arange(len(u)), indexing="ij")
        mats.append(O.distances(np.stack([u[i.ravel()], u[j.ravel()]], axis=1)).reshape(len(u), len(u)))
    DA, DB = mats
    rows, cols = np.tril_indices(len(ll), -1)

    def r_of(pa, pb):
        x, y = DA[pa[cols], pa[rows]], DB[pb[cols], pb[rows]]
        if np.var(x) == 0 or np.var(y) == 0:
            return np.nan
        return np.corrcoef(x, y)[0, 1]

    rng = np.random.default_rng(seed)
    stats = []
    for _ in range(permutations):
        mp = rng.permutation(len(u_b))
        mh = rng.permutation(len(u_a))
        stats.append(r_of(mh[pos_a], mp[pos_b]))
    return r_of(pos_a, pos_b), np.array(stats)


def _check_against_restatement(S, permutations, seeds):
    before = _state(S)
    for seed in seeds:
        r0, stats = _restated(S, permutations, seed)
        if np.all(np.abs(stats - r0) > 1e-9):
            break
    else:
        pytest.fail("no seed without a permuted r within 1e-9 of the observed r")
    assert np.all(np.abs(stats - r0) > 1e-9)
    res = S.hommola_cospeciation(permutations, seed=seed)
    assert _same_state(before, _state(S))
    assert abs(res.corr_coeff - r0) < 1e-12
    assert res.perm_stats.dtype == np.float64 and res.perm_stats.shape == (permutations,)
    assert np.max(np.abs(res.perm_stats - stats)) < 1e-12
    assert res.p_value == (np.count_nonzero(stats >= r0) + 1) / (permutations + 1)
    assert res.n_links == S.subset_n_links and res.permutations == permutations and res.seed == seed
    r, p, st = res
    assert (r, p) == (res.corr_coeff, res.p_value) and st is res.perm_stats
    return res


@pytest.mark.parametrize("which,permutations", [("gopher_louse", 999), ("fish_worm", 199)])
def test_fixtures_against_the_restatement(which, permutations):
    S = _slt(which)
    res = _check_against_restatement(S, permutations, range(1, 40))
    # the observed summary is linked_distances() reduced
    d = S.linked_distances()
    _check_moments(res.observed, d["TreeA"], d["TreeB"])
    # an identity row among permuted rows gives the observed sums, bit for bit
    gen = hommola_rows(*_universes(S), 99, 3, 1000)
    ident_a, ident_b = next(gen)
    ids_a, ids_b = next(gen)
    ids_a[57], ids_b[57] = ident_a[0], ident_b[0]
    m = S.TreeA._device_tree().compare_rows_host(S.TreeB._device_tree(), ids_a, ids_b)
    o = res.observed
    assert m[57]["n"] == o.n_pairs
    assert [float(m[57][k]) for k in _SUMS] == [getattr(o, k) for k in _SUMS]
    assert row_stats(m["n"], *(m[k] for k in _SUMS))[5][57] == res.corr_coeff


@pytest.fixture(scope="module")
def trees():
    pa, da = synth.random_binary_tree(3000, seed=7)
    pb, db = synth.random_binary_tree(2000, seed=8)
    return SuchTree((pa, da)), SuchTree((pb, db))


@pytest.mark.parametrize("m", [10, 60, 100, 300, 9000])
def test_rows_independent_of_position_batch_and_chunk(trees, m):
    A, B = trees
    dA, dB = A._device_tree(), B._device_tree()
    rng = np.random.default_rng(m)
    la, lb = np.asarray(A.leaf_node_ids, np.int64), np.asarray(B.leaf_node_ids, np.int64)
    X, Y = rng.choice(la, (100, m)), rng.choice(lb, (100, m))
    bx, by = X[0].copy(), Y[0].copy()
    X57, Y57 = X.copy(), Y.copy()
    X57[57], Y57[57] = bx, by
    X57[0], Y57[0] = X[57], Y[57]
    want = None
    # m = 9000: 4.0e7 pairs per row, more than one default chunk; at 8192 pairs per chunk that would be 5e5 chunks
    for chunk in ([0] if m == 9000 else [_capi.CLADE_TILE, 0]):
        alone = dA.compare_rows_host(dB, bx[None], by[None], chunk)
        b0 = dA.compare_rows_host(dB, X, Y, chunk)
        b57 = dA.compare_rows_host(dB, X57, Y57, chunk)
        want = alone.tobytes() if want is None else want
        assert alone.tobytes() == want
        assert b0[0:1].tobytes() == want and b57[57:58].tobytes() == want
        assert b0[57:58].tobytes() == b57[0:1].tobytes()
        assert np.delete(b0, [0, 57]).tobytes() == np.delete(b57, [0, 57]).tobytes()
    if m <= 300:
        x, _ = dA.triangle_host(bx)
        y, _ = dB.triangle_host(by)
        _check_moments(DistanceComparison.from_sums(*(alone[0][k] for k in _capi.PAIR_MOMENTS.names)), x, y)
    # degenerate rows: m < 2 and no rows
    for mm in (0, 1):
        e = dA.compare_rows_host(dB, np.zeros((3, mm), np.int64) + la[0], np.zeros((3, mm), np.int64) + lb[0])
        assert np.all(e["n"] == 0) and np.all(np.isnan(e["min_x"])) and np.all(e["sxx"] == 0)
    assert len(dA.compare_rows_host(dB, np.zeros((0, 5), np.int64), np.zeros((0, 5), np.int64))) == 0
    with pytest.raises(_capi.InvalidNodeError):
        dA.compare_rows_host(dB, np.full((2, 3), A.size + 4, np.int64), Y[:2, :3])


def test_large_rows_against_numpy():
    pa, da = synth.balanced_tree(8)
    pb, db = synth.random_binary_tree(6000, seed=3)
    A = SuchTree((pa, da, ["a%d" % i for i in range(256)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(6000)]))
    mat = np.zeros((256, 6000), dtype=np.int64)
    mat[np.random.default_rng(8).integers(0, 256, 6000), np.arange(6000)] = 1
    S = SuchLinkedTrees(A, B, pd.DataFrame(mat, index=list(A.leaves), columns=list(B.leaves)))
    gen = hommola_rows(*_universes(S), 4, 9, 10)
    parts = list(gen)
    ids_a, ids_b = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    dA, dB = A._device_tree(), B._device_tree()
    m = dA.compare_rows_host(dB, ids_a, ids_b)
    assert m["n"][0] == 6000 * 5999 // 2
    res = S.hommola_cospeciation(4, seed=9)
    for i in range(5):
        x, _ = dA.triangle_host(ids_a[i])
        y, _ = dB.triangle_host(ids_b[i])
        c = DistanceComparison.from_sums(*(m[i][k] for k in _capi.PAIR_MOMENTS.names))
        _check_moments(c, x, y)
        assert (res.corr_coeff if i == 0 else res.perm_stats[i - 1]) == c.pearson_r


def test_seeds_prefix_and_repeat():
    S = _slt("gopher_louse")
    seed_state = S._seed      # (the generator of sample_linked_distances)
    r30, r10 = S.hommola_cospeciation(30, seed=77), S.hommola_cospeciation(10, seed=77)
    assert r30.corr_coeff == r10.corr_coeff
    assert r30.perm_stats[:10].tobytes() == r10.perm_stats.tobytes()
    res = S.hommola_cospeciation(200)
    assert isinstance(res.seed, int)
    again = S.hommola_cospeciation(200, seed=res.seed)
    assert again.perm_stats.tobytes() == res.perm_stats.tobytes() and again.p_value == res.p_value
    zero = S.hommola_cospeciation(0, seed=1)
    assert zero.perm_stats.shape == (0,) and np.isnan(zero.p_value) and zero.corr_coeff == r10.corr_coeff
    assert S._seed == seed_state
    # sample_linked_distances continues as if no test had run
    S.sample_linked_distances(n=256, buckets=4, maxcycles=2)
    after_a = S._seed
    S._seed = seed_state
    S.hommola_cospeciation(50, seed=5)
    S.sample_linked_distances(n=256, buckets=4, maxcycles=2)
    assert S._seed == after_a != seed_state


def test_subset_semantics():
    S = _slt("fish_worm")
    B = S.TreeB
    root_links = S.subset_n_links
    for v in B.get_internal_nodes()[1:]:
        S.subset_b(int(v))
        if 20 <= S.subset_n_links < root_links:
            node = int(v)
            break
    assert S.subset_b_size < B.num_leaves
    _check_against_restatement(S, 99, range(1, 40))
    assert S.subset_b_root == node


def test_errors_and_nan():
    S = _slt("gopher_louse")
    with pytest.raises(ValueError):
        S.hommola_cospeciation(-1)
    # fewer than 3 links, universes of 16 leaves each
    pa, da = synth.balanced_tree(4)
    A2 = SuchTree((pa, da, ["a%d" % i for i in range(16)]))
    B2 = SuchTree((pa, da, ["b%d" % i for i in range(16)]))
    mat = np.zeros((16, 16), dtype=np.int64)
    mat[0, 0] = mat[5, 9] = 1
    F = SuchLinkedTrees(A2, B2, pd.DataFrame(mat, index=list(A2.leaves), columns=list(B2.leaves)))
    assert F.subset_n_links == 2 and F.subset_a_size == F.subset_b_size == 16
    with pytest.raises(ValueError, match="at least 3 links"):
        F.hommola_cospeciation(10, seed=1)
    # every link on one host: x is constant, r is NaN
    pa, da = synth.balanced_tree(4)
    pb, db = synth.balanced_tree(5)
    A = SuchTree((pa, da, ["a%d" % i for i in range(16)]))
    Bt = SuchTree((pb, db, ["b%d" % i for i in range(32)]))
    mat = np.zeros((16, 32), dtype=np.int64)
    mat[3, :] = 1
    N = SuchLinkedTrees(A, Bt, pd.DataFrame(mat, index=list(A.leaves), columns=list(Bt.leaves)))
    res = N.hommola_cospeciation(50, seed=1)
    assert np.isnan(res.corr_coeff) and np.isnan(res.p_value)
    assert res.perm_stats.shape == (50,) and np.all(np.isnan(res.perm_stats))
