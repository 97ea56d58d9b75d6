"""The swap null on the GPU: k_swap_chains (st_swap_null_tables, device 0) against the host restatement value for value --
word edges of the bit matrix, matrices of two rows and of a hub row, where the wave's batches are short, many short rows,
where they are long, chains shorter and longer than a batch, more chains than a workgroup has waves -- the table form of
the task kernels (st_dispersion_matrix_swap, st_partner_dispersion_swap_host) against the host bit for bit over the three
size classes, blocks of one and of three chains, and the facades."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare, synth

pytestmark = pytest.mark.gpu


def _rows(n_univ, sizes, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n_univ, k, replace=False)) for k in sizes]


def _matrices():
    rng = np.random.default_rng(77)
    out = {"univ%d" % n: (n, _rows(n, [n // 2, 3, 1, n - 1, 7, 2, n // 3, 5] * 3, n)) for n in (63, 64, 65, 200)}
    out["two_rows"] = (40, _rows(40, [11, 17], 1))
    out["short_rows"] = (200, _rows(200, rng.integers(1, 9, 300).tolist(), 2))
    out["hub"] = (120, _rows(120, [60] + [1] * 30 + [2] * 15, 3))      # the hub row holds half the links
    out["ones_and_full"] = (30, _rows(30, [1, 1, 30, 1, 0, 4, 1], 4))
    return out


MATRICES = _matrices()


def _both(n, rows, device_kwargs, **kw):
    want = _capi.swap_null_tables(rows, n, device=-1, **kw)
    got = _capi.swap_null_tables(rows, n, device=0, **kw)
    assert np.array_equal(got[1], want[1])
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[2] != want[2]))
    assert len(bad) == 0, "%s: rows %s differ; accepted got %s want %s" % (device_kwargs, bad[:5], got[2][bad[:5]], want[2][bad[:5]])
    return want


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_device_tables_equal_the_host(name):
    n, rows = MATRICES[name]
    for iterations in (0, 1, 63, 65, 1000):
        tables, offsets, accepted = _both(n, rows, (name, iterations), permutations=5, iterations=iterations, seed=31, stream=4)
        assert accepted[0] == 0 and np.array_equal(tables[0], np.concatenate(rows))
        if iterations == 1000 and name != "ones_and_full":
            assert accepted[1:].min() > 0 and (tables[1:] != tables[0]).any()      # the chains moved
    if name == "ones_and_full":      # the full row never swaps, the rows of one member do
        assert np.array_equal(tables[3][offsets[2]:offsets[3]], np.arange(30)) and accepted[1:].min() > 0


def test_more_chains_than_a_workgroup_and_a_later_begin():
    n, rows = MATRICES["univ200"]
    tables, _, accepted = _both(n, rows, "70 chains", permutations=69, iterations=500, seed=8, stream=1)
    assert len({t.tobytes() for t in tables}) == 70      # every chain its own
    late = _both(n, rows, "begin 37", permutations=9, begin=37, iterations=500, seed=8, stream=1)
    assert np.array_equal(late[0], tables[37:47]) and np.array_equal(late[2], accepted[37:47])


@pytest.mark.parametrize("form", ["SUCHTREE_AMD_SWAP_PLAIN", "SUCHTREE_AMD_SWAP_EARLY"])
def test_the_measurement_forms_of_the_chain_kernel(form, monkeypatch):
    """One trial per wave step, and the batched form that loads before the prefix is known: the same rows."""
    monkeypatch.setenv(form, "1")
    for name in ("univ65", "two_rows", "short_rows", "hub"):
        n, rows = MATRICES[name]
        _both(n, rows, (form, name), permutations=5, iterations=1000, seed=31, stream=4)


def test_default_iterations_and_structure():
    n, rows = MATRICES["short_rows"]
    links = sum(len(r) for r in rows)
    tables, offsets, accepted = _both(n, rows, "default", permutations=3, seed=5, stream=0)
    want = _capi.swap_null_tables(rows, n, permutations=3, iterations=max(1000, 10 * links), seed=5, device=-1)
    assert np.array_equal(tables, want[0]) and np.array_equal(accepted, want[2])
    degree = np.bincount(np.concatenate(rows), minlength=n)
    for t in tables:
        assert np.array_equal(np.bincount(t, minlength=n), degree)
        assert all((np.diff(t[offsets[r]:offsets[r + 1]].astype(np.int64)) > 0).all() for r in range(len(rows)))


SIZES = (2, 31, 32, 33, 64, 65, 300, 1, 0, 5)


@pytest.fixture(scope="module")
def record_case():
    """(D, sets, the host's records and accepted counts at 6 permutations) over a 512-position universe: computed once."""
    rng = np.random.default_rng(512)
    D = (rng.random((512, 512)) * 10.0 ** rng.integers(-2, 2, (512, 512))).astype(np.float32)
    sets = _rows(512, SIZES, 513)
    return D, sets, _capi.dispersion_matrix_swap(D, sets, 6, seed=19, iterations=3000, stream=2, device=-1)


@pytest.mark.parametrize("chunk", [0, 1, 3])
def test_records_equal_the_host_from_a_matrix(record_case, chunk):
    """chunk_tasks 1 and 3: blocks of one and of three chains."""
    D, sets, (want, want_accepted) = record_case
    got, accepted = _capi.dispersion_matrix_swap(D, sets, 6, seed=19, iterations=3000, stream=2, device=0, chunk_tasks=chunk)
    assert np.array_equal(accepted, want_accepted)
    bad = np.argwhere((got["pair_sum"].view(np.int64) != want["pair_sum"].view(np.int64))
                      | (got["nearest_sum"].view(np.int64) != want["nearest_sum"].view(np.int64)))
    assert len(bad) == 0, "%d records differ, first (set, p) %s" % (len(bad), bad[0])
    assert want[:, 1].tobytes() != want[:, 0].tobytes()


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links), links


@pytest.mark.parametrize("chunk", [0, 2])
def test_records_from_a_tree_and_the_tree_facade(record_case, chunk):
    """The same sets over the 512 leaves of a balanced tree: the matrix is written by the tree's distance kernels."""
    _, sets, _ = record_case
    tree = SuchTree(synth.balanced_tree(9), device=0)
    univ = tree._depth_first_leaves()
    n = len(univ)
    assert n == 512
    dev = tree._device_tree()
    D = dev.grid_host(univ, univ)[0].reshape(n, n).astype(np.float32)
    want, want_accepted = _capi.dispersion_matrix_swap(D, sets, 6, seed=11, iterations=None, stream=3, device=-1)
    got, accepted = dev.partner_dispersion_swap_host(univ, sets, 6, 11, None, 3, chunk_tasks=chunk)
    assert got.tobytes() == want.tobytes() and np.array_equal(accepted, want_accepted)
    if chunk:
        return
    # SuchTree.dispersion(null="swap") is the same matrix through the facade
    res = tree.dispersion([univ[s] for s in sets], permutations=6, seed=11, stream=3, keep_null=True, null="swap")
    assert res.null == "swap" and res.iterations == max(1000, 10 * sum(len(s) for s in sets)) and np.array_equal(res.swap_accepted, want_accepted)
    k = np.array([len(s) for s in sets])
    live = k >= 2
    kk = np.maximum(k, 2).astype(np.float64)
    assert np.array_equal(res.null_mpd[live], (want["pair_sum"][:, 1:] / (kk * (kk - 1))[:, None])[live])
    assert np.array_equal(res.mntd[live], (want["nearest_sum"][:, 0] / kk)[live]) and np.isnan(res.mpd[~live]).all()
    with pytest.raises(_capi.InvalidNodeError):
        dev.partner_dispersion_swap_host(np.append(univ[:-1], tree.size), sets, 6, 11, None, 3)


def _state(slt):
    return (slt.subset_a_root, slt.subset_b_root, slt.subset_a_size, slt.subset_b_size, slt.subset_a_leafs.tolist(), slt.subset_b_leafs.tolist(),
            slt.subset_rows.tolist(), slt.subset_columns.tolist(), slt.linklist.tolist(), slt._seed)


def test_partner_dispersion_swap_on_gopher_louse():
    slt, links = _slt("gopher_louse")
    before = _state(slt)
    one = slt.partner_dispersion(of="A", permutations=49, seed=3, min_partners=1, keep_null=True, null="swap")
    two = slt.partner_dispersion(of="A", permutations=49, seed=3, min_partners=2, keep_null=True, null="swap")
    assert _state(slt) == before
    counts = (links > 0).sum(axis=1)
    assert len(one) == int((counts >= 1).sum()) and len(two) == int((counts >= 2).sum()) and 0 < len(two) < len(one)
    assert np.array_equal(one.swap_accepted, two.swap_accepted) and one.swap_accepted[1:].min() > 0
    where = {leaf: i for i, leaf in enumerate(one.leaves.tolist())}
    for j, leaf in enumerate(two.leaves.tolist()):      # a reported row's columns do not depend on min_partners
        i = where[leaf]
        assert one.names[i] == two.names[j] and one.n[i] == two.n[j]
        assert one.null_mpd[i].tobytes() == two.null_mpd[j].tobytes() and one.null_mntd[i].tobytes() == two.null_mntd[j].tobytes()
        assert one.mpd_ses[i].tobytes() == two.mpd_ses[j].tobytes()
    default = slt.partner_dispersion(of="A", permutations=49, seed=3, min_partners=2, keep_null=True)
    assert default.null == "taxa.labels" and default.swap_accepted is None and default.mpd.tobytes() == two.mpd.tobytes()
    assert default.null_mpd.tobytes() != two.null_mpd.tobytes()
    small = [[0, 1], [1, 2]]
    assert compare.swap_null_tables(small, 3, permutations=2, seed=1, device=0)[0].tobytes() == compare.swap_null_tables(small, 3, permutations=2, seed=1)[0].tobytes()
