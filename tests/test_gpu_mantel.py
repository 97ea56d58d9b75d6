"""The Mantel kernels on the device against the host restatement of the same contract (st_mantel_codes, device = -1),
whose integers tests/test_mantel_host.py checks against the definition: every record and every moment compared with ==.
The smallest shapes that reach each path: the wave form at n = 3, 4, 63, 64; the row form at 65 (odd: the middle row
alone), 66 and 257 (a row longer than the workgroup); the large sort class at 2049; the first row above 32 KiB of LDS at
8193 and the largest row, 64 KiB, at 16384; chunks that cut a block of permutations and several blocks; the 128-bit carry
at the largest codes; the facades."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu


def _codes(n, seed, partial=True):
    """(x_sq, y, z): full-range int32 codes, x_sq symmetric with a diagonal that must not matter"""
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    draw = lambda k: rng.integers(-(1 << 31), 1 << 31, k, dtype=np.int64).astype(np.int32)      # noqa: E731
    a = draw(n * n).reshape(n, n)
    upper = np.triu(a, 1)
    x = upper + upper.T + np.diag(np.diag(a))
    return x, draw(m), (draw(m) if partial else None)


def _same(x, y, z, perms, seed=5, stream=3, chunk=0, what=""):
    want = _capi.mantel_codes(x, y, z, perms, seed, stream, -1)
    got = _capi.mantel_codes(x, y, z, perms, seed, stream, 0, chunk)
    assert got[0] == want[0], what
    assert got[1].tobytes() == want[1].tobytes(), what
    return got


@pytest.mark.parametrize("n", [3, 4, 63, 64])
def test_wave_form(n):
    x, y, z = _codes(n, n)
    _same(x, y, None, 9, what="simple")
    if n == 64:
        _same(x, y, z, 9, what="partial")
        _same(x, y, z, 9, chunk=3, what="partial, blocks of 3 permutations")


@pytest.mark.parametrize("n", [65, 66, 257])
def test_row_form(n):
    x, y, z = _codes(n, n)
    perms = 5 if n < 257 else 3
    _same(x, y, z if n == 66 else None, perms)
    if n != 66:
        _same(x, y, z, perms, what="partial")


@pytest.mark.parametrize("n", [65, 257])
def test_gather_form_kept_for_measurement_gives_the_same_records(n, monkeypatch):
    x, y, z = _codes(n, n)
    monkeypatch.setenv("SUCHTREE_AMD_MANTEL_GATHER", "1")
    _same(x, y, z, 4, what="partial, gathered")
    _same(x, y, None, 4, chunk=7, what="simple, gathered, chunks")


def test_large_sort_class():
    x, y, _ = _codes(2049, 1, partial=False)
    _same(x, y, None, 2)


def test_row_above_32_kib_of_lds():
    x, y, _ = _codes(8193, 2, partial=False)
    _same(x, y, None, 2)


def test_largest_row_of_64_kib():
    # n = 16384, the limit: the row form's dynamic LDS is 64 KiB beside its 128 static bytes, which only this size reaches.
    # Codes from the indices (drawing 2^28 of them would take longer than the call), one permutation.
    n = 16384
    idx = np.arange(n, dtype=np.uint32)
    x = (np.bitwise_xor.outer(idx, idx) * np.uint32(2654435761)).view(np.int32)
    y = (np.arange(n * (n - 1) // 2, dtype=np.uint32) * np.uint32(2246822519)).view(np.int32)
    _same(x, y, None, 1)


def test_chunks_cut_blocks_and_permutations():
    x, y, z = _codes(65, 7)
    one = _same(x, y, z, 7)
    for chunk in (5, 16, 40):      # 33 row pairs a permutation: blocks of 5, 8 and 8 permutations, chunks that end mid-row-pair
        got = _same(x, y, z, 7, chunk=chunk, what="chunk_tasks %d" % chunk)
        assert got[1].tobytes() == one[1].tobytes()


@pytest.mark.parametrize("sign", [1, -1])
def test_128_bit_carry(sign):
    n, top = 65, (1 << 31) - 1
    m = n * (n - 1) // 2
    x = np.full((n, n), top, dtype=np.int32)
    y = np.full(m, sign * top, dtype=np.int32)
    mom, rec = _same(x, y, y, 3)
    want = sign * m * top * top
    assert abs(want) > 1 << 63
    assert _capi.mantel_ints(rec, "sxy") == [want] * 4 and _capi.mantel_ints(rec, "sxz") == [want] * 4


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


FIELDS = ("corr_coeff", "p_value", "n", "n_pairs", "n_ge", "n_le", "n_abs_ge", "sxy", "sxz", "sx", "sy", "sz", "sxx", "syy", "szz", "syz",
          "shift_x", "shift_y", "shift_z", "seed", "permutations")


def _equal(a, b):
    for k in FIELDS:
        va, vb = getattr(a, k), getattr(b, k)
        assert va == vb or (va != va and vb != vb), k
    assert (a.perm_stats is None and b.perm_stats is None) or a.perm_stats.tobytes() == b.perm_stats.tobytes()


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_facade_device_and_host_agree_on_gopher_louse(method):
    slt = _slt("gopher_louse")
    ta, tb = slt.TreeA, slt.TreeB
    x = ta.pairwise_distances()
    rng = np.random.default_rng(3)
    y = x + rng.random(x.shape).round(2)
    y = (y + y.T) / 2
    z = compare.mantel_condensed(np.sqrt(x), "z")[0]      # (a third matrix, condensed)
    for third in (None, z):
        dev = compare.mantel(x, y, third, method=method, permutations=99, seed=11, keep_stats=True, device=0)
        host = compare.mantel(x, y, third, method=method, permutations=99, seed=11, keep_stats=True, device=None)
        _equal(dev, host)
    by_tree = ta.mantel(y, ta.leaf_node_ids, method=method, permutations=99, seed=11, keep_stats=True)
    _equal(by_tree, compare.mantel(x, y, method=method, permutations=99, seed=11, keep_stats=True, device=None))


@pytest.mark.parametrize("which,of,measure", [("gopher_louse", "A", "unifrac"), ("gopher_louse", "B", "beta_mpd"), ("fish_worm", "A", "unifrac"),
                                              ("fish_worm", "A", "beta_mntd"), ("fish_worm", "A", "phylosor")])
def test_phylosymbiosis_is_mantel_on_the_matrices_assembled_by_hand(which, of, measure):
    slt = _slt(which)
    before = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    got = slt.phylosymbiosis(of=of, measure=measure, permutations=49, seed=13, keep_stats=True)
    host = slt.phylosymbiosis(of=of, measure=measure, permutations=49, seed=13, keep_stats=True, device=None)
    _equal(got, host)
    if measure in ("unifrac", "phylosor"):
        parts = slt.partner_unifrac(of=of)
    else:
        parts = slt.partner_beta_dispersion(of=of, permutations=0, seed=0)
    own = slt.TreeA if of == "A" else slt.TreeB
    x = own.pairwise_distances(parts.leaves.tolist())
    want = compare.mantel(x, getattr(parts, measure), permutations=49, seed=13, alternative="greater", keep_stats=True, device=None)
    _equal(got, want)
    assert got.alternative == "greater" and got.measure == measure and got.names == parts.names and (got.leaves == parts.leaves).all()
    assert got.p_value == (got.n_ge + 1) / 50
    after = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    assert all((a == b).all() for a, b in zip(before, after))
    # the partial test, given the measure's own square root as a third matrix over the same rows
    control = np.sqrt(getattr(parts, measure))
    part = slt.phylosymbiosis(of=of, measure=measure, permutations=49, seed=13, control=control, keep_stats=True)
    _equal(part, compare.mantel(x, getattr(parts, measure), control, permutations=49, seed=13, alternative="greater", keep_stats=True, device=None))
