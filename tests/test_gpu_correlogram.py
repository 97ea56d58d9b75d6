"""The class-sum kernels on the device against the host restatement of the same contract (st_class_sums_codes, device =
-1), whose integers tests/test_correlogram_host.py checks against the definition: every sum compared by tobytes().  The
smallest shapes that reach each path: the wave form at n = 3, 4, 5 and 64 (with chunks); the row form at 65 (odd: the
middle row alone) and 66; rows of more than one step of a wave whose lengths are no multiple of 4 and whose first word
is misaligned in all four residues at 257 and 1027; slices shorter than four waves and a partial last slice; the
environment slice and the measured-against compare form; chunks that end inside a row pair and several blocks; 1, 2 and
64 classes, class 63 beside ST_CLASS_NONE, every pair in no class; sums past 2^32; one class that holds every pair of a
row (the accumulators' worst case); the large sort class at 2049; the first row above 32 KiB of LDS at 8193 and the
largest row at 16384; one column against the Mantel kernels on the indicator matrix; the facades -- which need the
trees' kernels for the matrices, so their host forms are here too."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu

S = 32      # kClassSlice (suchtree_amd/csrc/class_plan.h)
NONE = _capi.CLASS_NONE


def _case(n, seed, n_classes=5, none=0.2):
    """(y, cls): full-range int32 codes; classes below n_classes, a share `none` of the pairs in no class"""
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    y = rng.integers(-(1 << 31), 1 << 31, m, dtype=np.int64).astype(np.int32)
    cls = rng.integers(0, n_classes, m).astype(np.uint8)
    cls[rng.random(m) < none] = NONE
    return y, cls


def _same(y, cls, n_classes, perms, seed=5, stream=3, chunk=0, what=""):
    want = _capi.class_sums_codes(y, cls, n_classes, perms, seed, stream, -1)
    got = _capi.class_sums_codes(y, cls, n_classes, perms, seed, stream, 0, chunk)
    assert got.shape == want.shape == (perms + 1, n_classes)
    assert got.tobytes() == want.tobytes(), what
    return got


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65, 66])
def test_small_rows(n):
    y, c = _case(n, n)
    _same(y, c, 5, 9)


@pytest.mark.parametrize("n", [257, 1027])
def test_rows_longer_than_a_wave_step_and_misaligned(n):
    # rows i = 1 .. n - 1 start at word i (i - 1) / 2 of y: every residue mod 4, every length mod 4
    assert {(i * (i - 1) // 2) % 4 for i in range(1, n)} == {0, 1, 2, 3}
    y, c = _case(n, n)
    _same(y, c, 5, 3)


@pytest.mark.parametrize("perms", [1, 3, S, S + 1, 2 * S + 3])
def test_slices_shorter_than_four_waves_and_a_partial_last_slice(perms):
    y, c = _case(65, 11)
    _same(y, c, 5, perms - 1, what="%d rows of out" % perms)      # (perms rows: the observation is one of the slice's)
    _same(y, c, 5, perms, what="%d permutations" % perms)


def test_slice_length_changes_no_byte(monkeypatch):
    y, c = _case(65, 12)
    one = _same(y, c, 5, 2 * S + 3)
    for s in (1, 3, 8, 64):
        monkeypatch.setenv("SUCHTREE_AMD_CLASS_SLICE", str(s))
        assert _same(y, c, 5, 2 * S + 3, what="slice %d" % s).tobytes() == one.tobytes()


def test_the_compare_form_changes_no_byte(monkeypatch):
    y, c = _case(257, 19, 64)
    c[:3] = (63, NONE, 0)
    one = _same(y, c, 64, 5)
    monkeypatch.setenv("SUCHTREE_AMD_CLASS_ACC", "compare")
    assert _same(y, c, 64, 5, what="compare form").tobytes() == one.tobytes()


def test_wave_form_chunks_cut_blocks():
    y, c = _case(64, 8)
    one = _same(y, c, 5, 9)
    for chunk in (1, 3, 4, 7):      # blocks of `chunk` permutations: workgroups with fewer than four waves at work
        assert _same(y, c, 5, 9, chunk=chunk, what="chunk_tasks %d" % chunk).tobytes() == one.tobytes()


def test_chunks_cut_row_pairs_and_blocks(monkeypatch):
    y, c = _case(65, 7)
    one = _same(y, c, 5, 7)
    for s in (None, 2):      # 33 row pairs x 1 slice a block, then x several
        if s:
            monkeypatch.setenv("SUCHTREE_AMD_CLASS_SLICE", str(s))
        for chunk in (5, 16, 40):      # blocks of 5, 8 and 8 permutations, chunks that end inside a row pair's slices
            got = _same(y, c, 5, 7, chunk=chunk, what="chunk_tasks %d, slice %s" % (chunk, s))
            assert got.tobytes() == one.tobytes()


@pytest.mark.parametrize("n", [64, 66])
def test_class_counts(n):
    y, _ = _case(n, 13)
    m = len(y)
    one = _same(y, np.zeros(m, dtype=np.uint8), 1, 4)      # (one class holds every pair of every row: the contended accumulators)
    assert (one == int(y.sum(dtype=np.int64))).all()
    two = _same(y, _case(n, 14, 2, none=0.0)[1], 2, 4)
    assert (two.sum(axis=1) == int(y.sum(dtype=np.int64))).all()
    _same(y, _case(n, 16, 64)[1], 64, 4)
    c = np.random.default_rng(15).integers(60, 64, m).astype(np.uint8)
    c[np.random.default_rng(16).random(m) < 0.5] = NONE
    row = (n - 1) * (n - 2) // 2      # (class 63 and ST_CLASS_NONE side by side in the last row)
    c[row:row + 4] = (63, NONE, 63, NONE)
    top = _same(y, c, 64, 4)
    assert (top[:, :60] == 0).all() and top[0, 63] != 0
    none = _same(y, np.full(m, NONE, dtype=np.uint8), 64, 4)
    assert (none == 0).all()


@pytest.mark.parametrize("n", [64, 257])
@pytest.mark.parametrize("code", [(1 << 31) - 1, -(1 << 31)])
def test_sums_past_32_bits(code, n):
    m = n * (n - 1) // 2
    got = _same(np.full(m, code, dtype=np.int32), np.zeros(m, dtype=np.uint8), 1, 2)
    assert abs(code * m) > 1 << 32 and got.tolist() == [[code * m]] * 3


def test_one_class_holds_every_pair_of_a_row():
    # the classes by the larger object of the pair: under the identity all of row i lies in class i % 7, so every lane
    # of a wave adds to one class (test_class_counts has the one class that holds every pair under every permutation)
    n = 257
    y, _ = _case(n, 23)
    i, _j = np.tril_indices(n, -1)
    got = _same(y, (i % 7).astype(np.uint8), 7, 5)
    assert got[0].tolist() == [int(y[i % 7 == c].sum(dtype=np.int64)) for c in range(7)]


def test_large_sort_class():
    y, c = _case(2049, 1)
    _same(y, c, 5, 2)


def test_row_above_32_kib_of_lds():
    y, c = _case(8193, 2)
    _same(y, c, 5, 2)


def test_largest_row():
    # n = 16384, the limit: the row kernel's dynamic LDS is 64 KiB + 16 bytes, which only this size reaches, and the class
    # square 256 MiB.  Codes and classes from the indices (drawing 2^27 of them would take longer than the call), one
    # permutation.
    n = 16384
    k = np.arange(n * (n - 1) // 2, dtype=np.uint32)
    y = (k * np.uint32(2246822519)).view(np.int32)
    c = ((k * np.uint32(2654435761)) >> np.uint32(29)).astype(np.uint8)      # 0 .. 7
    c[c == 7] = NONE
    _same(y, c, 7, 1)


def test_a_column_is_the_mantel_sum_on_the_indicator():
    n = 66
    y, c = _case(n, 21, 4)
    got = _same(y, c, 4, 6)
    for h in range(4):
        x = compare.mantel_square((c == h).astype(np.int32), n)
        rec = _capi.mantel_codes(x, y, None, 6, 5, 3, 0)[1]
        assert _capi.mantel_ints(rec, "sxy") == got[:, h].tolist()


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


COLUMNS = ("breaks", "class_mid", "n_pairs", "sums_q", "corr_coeff", "n_ge", "n_le", "p_value", "p_corrected", "tested", "perm_stats")
FIELDS = ("n", "method", "permutations", "seed", "stream", "shift_y")


def _equal(a, b):
    for k in COLUMNS:
        va, vb = getattr(a, k), getattr(b, k)
        assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), k
    for k in FIELDS:
        assert getattr(a, k) == getattr(b, k), k


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_facades_agree_on_device_and_host(which, method):
    slt = _slt(which)
    own = slt.TreeA
    before = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    kw = dict(of="A", measure="unifrac", method=method, permutations=99, seed=13, keep_stats=True)
    got = slt.phylosymbiosis_correlogram(**kw)
    host = slt.phylosymbiosis_correlogram(device=None, **kw)
    _equal(got, host)
    # one row per class, the counts the same on the device and on the host
    parts = slt.partner_unifrac(of="A")
    n = len(parts.leaves)
    assert len(got) == int(np.ceil(1 + np.log2(n * (n - 1) // 2))) == len(got.to_dataframe()) and got.n == n
    assert got.n_ge.tolist() == host.n_ge.tolist() and got.n_le.tolist() == host.n_le.tolist()
    # the matrices assembled by hand
    x = own.pairwise_distances(parts.leaves.tolist())
    y = np.asarray(parts.unifrac, dtype=np.float64)
    for device in (None, 0):
        _equal(got, compare.mantel_correlogram(x, y, method=method, permutations=99, seed=13, keep_stats=True, device=device))
    assert got.leaves.tolist() == parts.leaves.tolist() and got.names == parts.names and got.measure == "unifrac"
    # the tree's own facade over the same leaves
    mine = own.mantel_correlogram(y, parts.leaves.tolist(), method=method, permutations=99, seed=13, keep_stats=True)
    _equal(got, mine)
    _equal(got, own.mantel_correlogram(y, parts.names, method=method, permutations=99, seed=13, keep_stats=True, device=None))
    assert mine.leaves.tolist() == parts.leaves.tolist() and mine.names == parts.names and mine.measure is None
    after = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    assert all((p == q).all() for p, q in zip(before, after))
    # the options reach the test: other classes, no cutoff, another correction
    few = slt.phylosymbiosis_correlogram(**dict(kw, n_classes=3, cutoff=False, correction="bonferroni", progressive=False))
    _equal(few, compare.mantel_correlogram(x, y, n_classes=3, cutoff=False, correction="bonferroni", progressive=False, method=method, permutations=99,
                                           seed=13, keep_stats=True, device=None))
    assert len(few) == 3 and few.tested[0] and few.tested[-1]      # (the end classes hold min(x) and max(x): neither empty nor all)
    for bad in ({"of": "C"}, {"measure": "jaccard"}, {"method": "kendall"}, {"correction": "fdr"}, {"permutations": -1}, {"n_classes": 65}):
        with pytest.raises(ValueError):
            slt.phylosymbiosis_correlogram(**dict(kw, **bad))
    with pytest.raises(ValueError, match="not over"):
        own.mantel_correlogram(y[:3], parts.leaves.tolist())
