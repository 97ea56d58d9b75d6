"""The host side of the quartet comparison (no GPU): st_quartet_positions(device = -1) -- the unranking of all C(m,4)
quartets and the seeded draw -- against plain Python, its argument errors, QuartetComparison's statistics, and the host
code under the address / undefined-behaviour sanitizers."""
import ctypes
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.compare import QuartetComparison, quartet_positions

M64 = (1 << 64) - 1


def py_mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_draw(seed, k, m):
    chosen, out = [], []
    for j in range(4):
        u = py_mix((seed + (4 * k + j + 1) * 0x9E3779B97F4A7C15) & M64)
        p = (u * (m - j)) >> 64
        for q in sorted(chosen):
            if p >= q:
                p += 1
        chosen.append(p)
        out.append(p)
    return out


# ---- unranking ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(4, 13))
def test_unranking_is_the_colexicographic_order(m):
    got = quartet_positions(m)
    want = sorted(itertools.combinations(range(m), 4), key=lambda t: t[::-1])
    assert got.dtype == np.int32 and got.shape == (math.comb(m, 4), 4)
    assert got.tolist() == [list(t) for t in want]


@pytest.mark.parametrize("p", [4, 5, 1000, 65535])
def test_unranking_at_the_block_edges(p):
    k = math.comb(p, 4)
    assert quartet_positions(65536, begin=k, count=1).tolist() == [[0, 1, 2, p]]
    assert quartet_positions(65536, begin=k - 1, count=1).tolist() == [[p - 4, p - 3, p - 2, p - 1]]
    # the same quartets with exactly p + 1 leaves: the last block of a smaller list
    assert quartet_positions(p + 1, begin=k, count=1).tolist() == [[0, 1, 2, p]]


def test_the_last_quartet_of_65536_leaves():
    total = math.comb(65536, 4)
    assert total < 1 << 60
    assert quartet_positions(65536, begin=total - 1).tolist() == [[65532, 65533, 65534, 65535]]
    assert len(quartet_positions(65536, begin=total)) == 0


def test_a_range_that_begins_inside_a_block():
    full = quartet_positions(30)
    k0 = math.comb(25, 4) + 777
    assert np.array_equal(quartet_positions(30, begin=k0, count=1000), full[k0:k0 + 1000])
    # far out, against Python's own unranking
    k0 = math.comb(60000, 4) + math.comb(31000, 3) + 5
    got = quartet_positions(65536, begin=k0, count=1000)

    def unrank(k):
        out = []
        for r in (4, 3, 2, 1):
            p = int(round((math.factorial(r) * k) ** (1.0 / r))) + r
            while math.comb(p, r) > k:
                p -= 1
            out.append(p)
            k -= math.comb(p, r)
        return out[::-1]
    assert got.tolist() == [unrank(k0 + i) for i in range(1000)]


# ---- the draw -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, M64])
@pytest.mark.parametrize("m", [4, 5, 1000, 2 ** 31 - 1])
def test_draw_equals_the_python_restatement(seed, m):
    got = quartet_positions(m, samples=2000, seed=seed)
    assert got.tolist() == [py_draw(seed, k, m) for k in range(2000)]
    s = np.sort(got, axis=1)
    assert (s[:, 1:] > s[:, :-1]).all() and s.min() >= 0 and s.max() < m
    if m == 4:
        assert (s == np.arange(4)).all() and len({tuple(r) for r in got.tolist()}) == 24
    # the prefix property: quartet k does not depend on where a range begins or ends
    assert np.array_equal(quartet_positions(m, samples=500, seed=seed), got[:500])
    assert np.array_equal(quartet_positions(m, samples=2000, seed=seed, begin=1234), got[1234:])
    assert np.array_equal(quartet_positions(m, samples=10 ** 9, seed=seed, begin=1999, count=1), got[1999:])


def test_draw_at_the_end_of_the_index_range():
    k0 = (1 << 62) - 3
    got = quartet_positions(1000, samples=1 << 62, seed=5, begin=k0)
    assert got.tolist() == [py_draw(5, k0 + i, 1000) for i in range(3)]


def test_draw_reaches_every_ordered_tuple_evenly():
    got = quartet_positions(5, samples=200_000, seed=7)
    counts = np.unique(got @ np.array([125, 25, 5, 1]), return_counts=True)[1]
    # 120 ordered tuples, 1666.7 expected each: binomial sd 40.6, and +-6 sd is never met by chance
    assert len(counts) == 120 and counts.min() > 1666.7 - 6 * 40.6 and counts.max() < 1666.7 + 6 * 40.6


# ---- argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError):
        quartet_positions(3, samples=1)                      # m = 3 with a count
    with pytest.raises(ValueError):
        quartet_positions(3, begin=0, count=1)
    assert quartet_positions(3).shape == (0, 4) and quartet_positions(3, samples=0).shape == (0, 4)
    with pytest.raises(ValueError):
        quartet_positions(65537)
    with pytest.raises(ValueError):
        quartet_positions(65537, begin=0, count=1)
    with pytest.raises(ValueError):
        quartet_positions(10, begin=200, count=11)           # C(10,4) = 210
    with pytest.raises(ValueError):
        quartet_positions(2 ** 31, samples=1)
    with pytest.raises(ValueError):
        quartet_positions(10, samples=1, begin=1 << 62, count=1)
    L = _capi.load()
    assert L.st_quartet_positions(-1, 0, 0, 10, 0, 5, None) == _capi.ST_ERR_ARG      # a NULL output
    assert L.st_quartet_positions(-1, 7, 0, 10, 0, 0, None) == _capi.ST_ERR_ARG      # a mode that does not exist
    assert L.st_quartet_positions(-1, 0, 0, 10, 0, 0, None) == _capi.ST_OK
    out = (ctypes.c_int32 * 4)()
    assert L.st_quartet_positions(-2, 0, 0, 10, 0, 1, out) == _capi.ST_ERR_ARG


# ---- statistics -----------------------------------------------------------------------------------------------------
def test_quartet_comparison_statistics():
    table = np.array([[50, 3, 2, 1], [4, 20, 5, 0], [6, 7, 10, 2], [1, 0, 3, 4]])
    c = QuartetComparison.from_table(table, n_leaves=30, mode="sample", seed=9)
    assert c.n == 118 and c.agree == 80 and c.unresolved == 1 + 0 + 2 + 1 + 0 + 3 + 4
    assert c.similarity == 80 / 118 and c.distance == 1 - 80 / 118
    assert c.stderr == math.sqrt((80 / 118) * (1 - 80 / 118) / 118)
    assert c.table.dtype == np.int64 and c.seed == 9 and c.n_leaves == 30
    a = QuartetComparison.from_table(table, n_leaves=30, mode="all")
    assert a.stderr == 0.0 and a.distance == c.distance
    empty = QuartetComparison.from_table(np.zeros((4, 4)))
    assert empty.n == 0 and math.isnan(empty.similarity) and math.isnan(empty.distance) and empty.mode == "given"
    with pytest.raises(ValueError):
        QuartetComparison(n=5, table=table)
    with pytest.raises(ValueError):
        QuartetComparison.from_table(np.zeros((3, 4)))


def test_merge_adds_the_tables():
    rng = np.random.default_rng(2)
    ta, tb = rng.integers(0, 1000, (4, 4)), rng.integers(0, 1000, (4, 4))
    a = QuartetComparison.from_table(ta, n_leaves=100, mode="sample", seed=4)
    b = QuartetComparison.from_table(tb, n_leaves=100, mode="sample", seed=4)
    c = QuartetComparison.merge(a, b)
    assert np.array_equal(c.table, ta + tb) and c.n == a.n + b.n and c.agree == a.agree + b.agree
    assert (c.n_leaves, c.mode, c.seed) == (100, "sample", 4)
    d = QuartetComparison.merge(a, QuartetComparison.from_table(tb, n_leaves=7, mode="all"))
    assert (d.n_leaves, d.mode, d.seed) == (None, "given", None) and d.n == c.n


def test_too_many_quartets_to_enumerate_ask_for_a_sample():
    p, d = synth.random_binary_tree(70_000, seed=1)
    T = SuchTree((p, d))
    ids = np.arange(2000, dtype=np.int64) * 2
    assert math.comb(2000, 4) > 1 << 36
    with pytest.raises(ValueError, match="samples="):
        T.compare_quartets(T, leaves=(ids, ids))               # raised before either tree is uploaded
    ids = np.arange(65537, dtype=np.int64) * 2
    with pytest.raises(ValueError, match="samples="):
        T.compare_quartets(T, leaves=(ids, ids))
    with pytest.raises(ValueError):
        T.compare_quartets(T, leaves=(ids[:3], ids[:3]), samples=5)
    with pytest.raises(ValueError):
        T.compare_quartets(T, leaves=(ids, ids), quartets=(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int64)))
    with pytest.raises(ValueError):
        T.compare_quartets(T, samples=5, quartets=(np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int64)))
    with pytest.raises(TypeError):
        T.compare_quartets(T, quartets=[("a", "b", "c")])
    assert T._dev_tree is None


# ---- sanitizers -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_quartet_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_quartets")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_quartets.cpp"),
                           os.path.join(ROOT, "suchtree_amd", "csrc", "quartet_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize quartets ok" in out.stdout
