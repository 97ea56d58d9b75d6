"""The group-sum kernels on the device against the host restatement of the same contract (st_group_sums_codes, device =
-1), whose integers tests/test_group_tests_host.py checks against the definition: every sum compared by tobytes().  The
smallest shapes that reach each path: the wave form at n = 3, 4, 5 and 64 (with chunks, and four passes of columns at
256 groups); the row form at 65 (odd: the middle row alone) and 66; rows of more than one step of a wave whose lengths
are no multiple of 4 and whose first word is misaligned in all four residues at 257 and 1027; slices shorter than four
waves and a partial last slice; chunks that end inside a row pair and several blocks; the byte compare at labels 254 /
255; sums past 2^32; the large sort class at 2049; the first row above 32 KiB of LDS at 8193 and the largest row, 64
KiB, at 16384; one column against the Mantel kernels on the indicator matrix; the facades -- which need the trees'
kernels for the matrix, so their host forms are here too."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu

S = 64      # kGroupSlice (suchtree_amd/csrc/group_plan.h)


def _case(n, seed, n_groups=5):
    """(y, group): full-range int32 codes and labels below n_groups"""
    rng = np.random.default_rng(seed)
    y = rng.integers(-(1 << 31), 1 << 31, n * (n - 1) // 2, dtype=np.int64).astype(np.int32)
    return y, rng.integers(0, n_groups, n).astype(np.uint8)


def _same(y, group, n_groups, perms, seed=5, stream=3, chunk=0, what=""):
    want = _capi.group_sums_codes(y, group, n_groups, perms, seed, stream, -1)
    got = _capi.group_sums_codes(y, group, n_groups, perms, seed, stream, 0, chunk)
    assert got.shape == want.shape == (perms + 1, n_groups)
    assert got.tobytes() == want.tobytes(), what
    return got


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 66])
def test_small_rows(n):
    y, g = _case(n, n)
    _same(y, g, 5, 9)


@pytest.mark.parametrize("n", [257, 1027])
def test_rows_longer_than_a_wave_step_and_misaligned(n):
    # rows i = 1 .. n - 1 start at word i (i - 1) / 2 of y: every residue mod 4, every length mod 4
    assert {(i * (i - 1) // 2) % 4 for i in range(1, n)} == {0, 1, 2, 3}
    y, g = _case(n, n)
    _same(y, g, 5, 3)


@pytest.mark.parametrize("perms", [1, 3, S, S + 1, 2 * S + 3])
def test_slices_shorter_than_four_waves_and_a_partial_last_slice(perms):
    y, g = _case(65, 11)
    _same(y, g, 5, perms - 1, what="%d rows of out" % perms)      # (perms rows: the observation is one of the slice's)
    _same(y, g, 5, perms, what="%d permutations" % perms)


def test_slice_length_changes_no_byte(monkeypatch):
    y, g = _case(65, 12)
    one = _same(y, g, 5, 2 * S + 3)
    for s in (1, 3, 16, 64):
        monkeypatch.setenv("SUCHTREE_AMD_GROUP_SLICE", str(s))
        assert _same(y, g, 5, 2 * S + 3, what="slice %d" % s).tobytes() == one.tobytes()


def test_wave_form_chunks_cut_blocks():
    y, g = _case(64, 8)
    one = _same(y, g, 5, 9)
    for chunk in (1, 3, 4, 7):      # blocks of `chunk` permutations: workgroups with fewer than four waves at work
        assert _same(y, g, 5, 9, chunk=chunk, what="chunk_tasks %d" % chunk).tobytes() == one.tobytes()


def test_chunks_cut_row_pairs_and_blocks(monkeypatch):
    y, g = _case(65, 7)
    one = _same(y, g, 5, 7)
    for s in (None, 2):      # 33 row pairs x 1 slice a block, then x several
        if s:
            monkeypatch.setenv("SUCHTREE_AMD_GROUP_SLICE", str(s))
        for chunk in (5, 16, 40):      # blocks of 5, 8 and 8 permutations, chunks that end inside a row pair's slices
            got = _same(y, g, 5, 7, chunk=chunk, what="chunk_tasks %d, slice %s" % (chunk, s))
            assert got.tobytes() == one.tobytes()


@pytest.mark.parametrize("n", [64, 66])
def test_group_counts_at_the_ends_of_the_byte(n):
    y, _ = _case(n, 13)
    one = _same(y, np.zeros(n, dtype=np.uint8), 1, 4)
    assert (one == int(y.sum(dtype=np.int64))).all()
    _same(y, _case(n, 14, 2)[1], 2, 4)
    _same(y, _case(n, 16, 65)[1], 65, 4)      # (the wave form: a second pass of columns for one label)
    g = np.random.default_rng(15).integers(250, 256, n).astype(np.uint8)
    g[:4] = (254, 255, 254, 255)
    top = _same(y, g, 256, 4)
    assert (top[:, :250] == 0).all() and top[0, 254] != 0 and top[0, 255] != 0


@pytest.mark.parametrize("n", [64, 257])
@pytest.mark.parametrize("code", [(1 << 31) - 1, -(1 << 31)])
def test_sums_past_32_bits(code, n):
    m = n * (n - 1) // 2
    got = _same(np.full(m, code, dtype=np.int32), np.zeros(n, dtype=np.uint8), 1, 2)
    assert abs(code * m) > 1 << 32 and got.tolist() == [[code * m]] * 3


def test_large_sort_class():
    y, g = _case(2049, 1)
    _same(y, g, 5, 2)


def test_row_above_32_kib_of_lds():
    y, g = _case(8193, 2)
    _same(y, g, 5, 2)


def test_largest_row_of_64_kib():
    # n = 16384, the limit: the row kernel's dynamic LDS is 64 KiB, which only this size reaches.  Codes from the indices
    # (drawing 2^27 of them would take longer than the call), one permutation.
    n = 16384
    y = (np.arange(n * (n - 1) // 2, dtype=np.uint32) * np.uint32(2246822519)).view(np.int32)
    g = ((np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(29)).astype(np.uint8)
    _same(y, g, 8, 1)


def test_a_column_is_the_mantel_sum_on_the_indicator():
    n = 66
    y, g = _case(n, 21, 4)
    got = _same(y, g, 4, 6)
    for h in range(4):
        x = ((g[:, None] == h) & (g[None, :] == h)).astype(np.int32)
        rec = _capi.mantel_codes(x, y, None, 6, 5, 3, 0)[1]
        assert _capi.mantel_ints(rec, "sxy") == got[:, h].tolist()


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


FIELDS = ("statistic", "p_value", "n_ge", "n", "n_groups", "group_sizes", "labels", "within_q", "shift", "method", "permutations", "seed", "r2")


def _equal(a, b):
    for k in FIELDS:
        va, vb = getattr(a, k), getattr(b, k)
        assert va == vb or (va != va and vb != vb), k
    assert a.perm_stats.tobytes() == b.perm_stats.tobytes()


def _two_clades(tree):
    """the two disjoint internal clades whose smaller one is the largest (a caterpillar has no balanced split)"""
    under = {int(v): set(tree.get_leaves(v).tolist()) for v in tree.get_internal_nodes() if int(v) != tree.root_node}
    pairs = [(min(len(under[a]), len(under[b])), len(under[a]) + len(under[b]), a, b) for a in under for b in under if a < b and not under[a] & under[b]]
    return max(pairs)[2:]


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("test", ["permanova", "anosim"])
def test_facades_agree_on_device_and_host(which, test):
    slt = _slt(which)
    own = slt.TreeA
    before = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    a, b = _two_clades(own)
    kw = dict(of="A", groups=[a, b], measure="unifrac", test=test, permutations=99, seed=13, keep_stats=True)
    got = slt.partner_group_differences(**kw)
    host = slt.partner_group_differences(device=None, **kw)
    _equal(got, host)
    # the matrix assembled by hand
    parts = slt.partner_unifrac(of="A")
    in_a, in_b = set(own.get_leaves(a).tolist()), set(own.get_leaves(b).tolist())
    rows = [k for k, leaf in enumerate(parts.leaves.tolist()) if leaf in in_a or leaf in in_b]
    square = compare.mantel_square(np.arange(len(parts.unifrac)), len(parts.leaves))      # (the index of every pair)
    d = np.asarray(parts.unifrac, dtype=np.float64)[square[np.ix_(rows, rows)]]
    np.fill_diagonal(d, 0.0)
    grouping = [a if parts.leaves[k] in in_a else b for k in rows]
    fn = compare.permanova if test == "permanova" else compare.anosim
    _equal(got, fn(d, grouping, permutations=99, seed=13, keep_stats=True, device=None))
    _equal(got, fn(d, grouping, permutations=99, seed=13, keep_stats=True, device=0))
    assert got.leaves.tolist() == [int(parts.leaves[k]) for k in rows] and got.names == [parts.names[k] for k in rows]
    assert got.dropped.tolist() == [int(v) for k, v in enumerate(parts.leaves.tolist()) if k not in set(rows)]
    assert got.measure == "unifrac" and got.p_value == (got.n_ge + 1) / 100
    after = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    assert all((x == y).all() for x, y in zip(before, after))
    # a mapping from names gives the same test; overlapping clades raise and name both
    by_name = {own.leaf_nodes[int(leaf)]: (a if leaf in in_a else b) for leaf in got.leaves.tolist()}
    _equal(got, slt.partner_group_differences(**dict(kw, groups=by_name)))
    with pytest.raises(ValueError, match="overlap"):
        slt.partner_group_differences(**dict(kw, groups=[a, b, own.root_node]))
