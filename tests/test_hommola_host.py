"""Hommola's permutation test without a GPU: the new export and its argument errors, the rows of the test against an
independent restatement of scikit-bio's draw order, the p-value rule, argument errors of the public method, and the
registers of the new kernel."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT, golden_path
from suchtree_amd import SuchTree, _capi, build as st_build, synth
from suchtree_amd.compare import hommola_pvalue, hommola_rows
from suchtree_amd.linked import SuchLinkedTrees


@pytest.fixture(scope="module")
def lib():
    st_build.build()
    return _capi.load()


def test_rows_symbol_is_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    assert re.search(r"\bint\s+st_compare_rows_host\s*\(", header)
    assert "st_compare_rows_host" in _capi.SYMBOLS
    assert getattr(lib, "st_compare_rows_host") is not None
    assert lib.st_api_version() == 7 == _capi.API_VERSION


def test_rows_argument_errors_without_a_gpu(lib):
    ids = np.arange(12, dtype=np.int64).reshape(3, 4)
    out = np.zeros(3, dtype=_capi.PAIR_MOMENTS)
    b = ctypes.c_int64(0)
    p = _capi._ptr

    def call(tx, ty, ix, iy, n_rows, m, chunk, o):
        return lib.st_compare_rows_host(tx, ty, ix, iy, n_rows, m, chunk, o, ctypes.byref(b))

    assert call(None, None, p(ids), p(ids), 3, 4, 0, p(out)) == _capi.ST_ERR_ARG      # NULL trees
    assert "tree" in _capi.last_error()
    assert call(None, None, None, p(ids), 3, 4, 0, p(out)) == _capi.ST_ERR_ARG        # NULL ids
    assert call(None, None, p(ids), None, 3, 4, 0, p(out)) == _capi.ST_ERR_ARG
    assert "ids" in _capi.last_error()
    assert call(None, None, p(ids), p(ids), 3, 4, 0, None) == _capi.ST_ERR_ARG        # NULL out
    assert call(None, None, p(ids), p(ids), -1, 4, 0, p(out)) == _capi.ST_ERR_ARG     # negative sizes
    assert call(None, None, p(ids), p(ids), 3, -4, 0, p(out)) == _capi.ST_ERR_ARG
    assert "n_rows < 0 or m < 0" in _capi.last_error()
    for chunk in (_capi.CLADE_TILE + 1, -_capi.CLADE_TILE, 100):                      # bad chunk sizes
        assert call(None, None, p(ids), p(ids), 3, 4, chunk, p(out)) == _capi.ST_ERR_ARG
        assert "chunk_pairs" in _capi.last_error()


def _restated(u_a, u_b, pos_a, pos_b, permutations, seed):
    """scikit-bio's draw order, written out: row 0 the links, then per permutation mp (guest), mh (host)."""
    rng = np.random.default_rng(seed)
    rows_a, rows_b = [u_a[pos_a]], [u_b[pos_b]]
    for _ in range(permutations):
        mp = rng.permutation(len(u_b))
        mh = rng.permutation(len(u_a))
        rows_b.append(np.array([u_b[mp[q]] for q in pos_b]))
        rows_a.append(np.array([u_a[mh[q]] for q in pos_a]))
    return np.array(rows_a), np.array(rows_b)


def _collect(gen):
    parts = list(gen)
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts]), parts


def test_rows_follow_the_draw_order():
    rng = np.random.default_rng(5)
    u_a = rng.choice(1000, 13, replace=False).astype(np.int64)
    u_b = rng.choice(1000, 9, replace=False).astype(np.int64)
    L = 20
    pos_a, pos_b = rng.integers(0, 13, L), rng.integers(0, 9, L)
    want_a, want_b = _restated(u_a, u_b, pos_a, pos_b, 30, 1234)
    for batch in (1, 7, 30, 1000):
        got_a, got_b, parts = _collect(hommola_rows(u_a, u_b, pos_a, pos_b, 30, 1234, batch))
        assert parts[0][0].shape == (1, L)                      # row 0 alone, first
        assert all(len(a) <= batch for a, _ in parts[1:])
        assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
        assert got_a.dtype == np.int64 and got_a.flags.c_contiguous
    # row 0 is the identity
    assert np.array_equal(got_a[0], u_a[pos_a]) and np.array_equal(got_b[0], u_b[pos_b])
    # every row relabels through one permutation of each universe: links on one leaf stay on one leaf, distinct leaves
    # stay distinct, and every label is in the universe
    for p in range(1, 31):
        for got, u, pos in ((got_a, u_a, pos_a), (got_b, u_b, pos_b)):
            image = {}
            for q, v in zip(pos, got[p]):
                assert image.setdefault(int(q), int(v)) == int(v)
            assert len(set(image.values())) == len(image) and set(image.values()) <= set(u.tolist())
    # the prefix property
    pre_a, pre_b, _ = _collect(hommola_rows(u_a, u_b, pos_a, pos_b, 10, 1234, 4))
    assert np.array_equal(pre_a, got_a[:11]) and np.array_equal(pre_b, got_b[:11])
    # no permutations: row 0 only
    z_a, z_b, parts = _collect(hommola_rows(u_a, u_b, pos_a, pos_b, 0, 1234, 4))
    assert len(parts) == 1 and np.array_equal(z_a[0], u_a[pos_a])


def test_pvalue_rule():
    assert hommola_pvalue(0.5, np.array([0.1, 0.5, 0.7, 0.2])) == 3 / 5       # a tie counts
    assert hommola_pvalue(0.5, np.array([0.1, np.nan, 0.7])) == 2 / 4         # NaN does not
    assert hommola_pvalue(0.9, np.array([0.1, 0.2])) == 1 / 3
    assert hommola_pvalue(-1.0, np.array([-1.0, -0.5])) == 1.0
    assert np.isnan(hommola_pvalue(0.5, np.empty(0)))                         # permutations = 0
    assert np.isnan(hommola_pvalue(float("nan"), np.array([0.1, 0.2])))       # NaN observed r


def _gopher():
    d = golden_path("gopher_louse")
    return SuchLinkedTrees(SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree"), pd.read_csv(d + "/links.csv", index_col=0))


def _balanced_linked(links):
    """Two balanced 16-leaf trees linked by (TreeA name, TreeB name) pairs."""
    pa, da = synth.balanced_tree(4)
    pb, db = synth.balanced_tree(4)
    A = SuchTree((pa, da, ["a%d" % i for i in range(16)]))
    B = SuchTree((pb, db, ["b%d" % i for i in range(16)]))
    mat = pd.DataFrame(0, index=list(A.leaves), columns=list(B.leaves))
    for a, b in links:
        mat.loc[a, b] = 1
    return SuchLinkedTrees(A, B, mat)


def test_public_method_argument_errors_before_any_launch():
    S = _gopher()
    for bad in (-1, 2.5, "10", True, None):
        with pytest.raises(ValueError, match="permutations"):
            S.hommola_cospeciation(permutations=bad)
    # fewer than 3 links, universes of 16 leaves each
    S = _balanced_linked([("a0", "b0"), ("a5", "b9")])
    assert S.subset_n_links == 2 and S.subset_a_size == S.subset_b_size == 16
    with pytest.raises(ValueError, match="at least 3 links"):
        S.hommola_cospeciation(99, seed=1)
    # 3 links on a TreeB clade of 2 leaves: the guest universe is too small
    probe = _balanced_linked([])
    B = probe.TreeB
    clade = next(int(v) for v in B.get_internal_nodes() if len(probe._leaves_below(B, v)) == 2)
    name_of = {int(i): n for n, i in B.leaves.items()}
    n1, n2 = (name_of[int(v)] for v in probe._leaves_below(B, clade))
    S = _balanced_linked([("a0", n1), ("a1", n1), ("a2", n2)])
    S.subset_b(clade)
    assert S.subset_n_links == 3 and S.subset_b_size == 2
    before, seed_state = S.linklist.copy(), S._seed
    with pytest.raises(ValueError, match="at least 3 leaves"):
        S.hommola_cospeciation(99, seed=1)
    assert np.array_equal(before, S.linklist) and S.subset_b_root == clade and S._seed == seed_state


def test_rows_memory_follows_the_links_not_the_universes():
    """A 100,000-leaf universe with 30 links: one batch holds 300 x 30 ids per tree, and one permutation of each
    universe (0.8 MB) exists at a time.  Keeping whole permutations per row would take 480 MB."""
    import tracemalloc
    rng = np.random.default_rng(3)
    u_a, u_b = np.arange(100_000, dtype=np.int64) * 2, np.arange(100_000, dtype=np.int64) * 2 + 1
    pos_a, pos_b = rng.integers(0, 100_000, 30), rng.integers(0, 100_000, 30)
    tracemalloc.start()
    try:
        rows = sum(len(a) for a, _ in hommola_rows(u_a, u_b, pos_a, pos_b, 300, 7, (1 << 23) // 30))
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert rows == 301
    assert peak < 8 << 20, peak


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_row_kernels_compile_for_gfx950_without_spills(tmp_path):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-DST_CANOPY_PART=3", "-o", str(tmp_path / "unit.o"),
                          os.path.join(ROOT, "suchtree_amd", "csrc", "launch_canopy.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "SrcRows" in out.stderr
    for m in re.finditer(r"VGPRs Spill: (\d+)", out.stderr):
        assert int(m.group(1)) == 0
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "main.o"), os.path.join(ROOT, "suchtree_amd", "csrc", "suchtree_hip.hip")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    name, seen = None, False
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name and "k_row_blocks" in name:
            seen = True
            assert int(m.group(1)) == 0
    assert seen
