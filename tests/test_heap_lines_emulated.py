"""Heap lines of perfect trees (tree_prep.cpp: prepare_heap_lines) on the CPU: which trees are admitted, the table sizes,
and the pair function of k_canopy_ilp_heap over the two tables (tests/emu/heap_emulator.cpp) against the oracle, by bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, oracle_both
from suchtree_amd import synth


class HeapEmulator:
    def __init__(self):
        emu_dir = os.path.join(ROOT, "tests", "emu")
        lib = os.path.join(emu_dir, "libst_heap_emu.so")
        srcs = [os.path.join(emu_dir, "heap_emulator.cpp"), os.path.join(ROOT, "suchtree_amd", "csrc", "tree_prep.cpp")]
        deps = srcs + [os.path.join(ROOT, "suchtree_amd", "csrc", h) for h in ("tree_prep.h", "pair_math.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            tmp = "%s.tmp.%d" % (lib, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + srcs)
            os.replace(tmp, lib)
        self.lib = ctypes.CDLL(lib)
        self.lib.heap_emu_last_error.restype = ctypes.c_char_p

    @staticmethod
    def _tree(parent, dist):
        return np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(dist, np.float32)

    def prepare(self, parent, dist):
        """(admitted, floats of heap_lines, floats of heap_dist, levels)"""
        parent, dist = self._tree(parent, dist)
        sizes = np.zeros(3, np.int64)
        rc = self.lib.heap_emu_prepare(parent.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_int64(len(parent)), sizes.ctypes.data_as(ctypes.c_void_p))
        assert rc in (0, 2), self.lib.heap_emu_last_error().decode()
        return rc == 0, int(sizes[0]), int(sizes[1]), int(sizes[2])

    def run(self, parent, dist, pairs):
        parent, dist = self._tree(parent, dist)
        pairs = np.ascontiguousarray(pairs, np.int64)
        d, m = np.zeros(len(pairs)), np.zeros(len(pairs), np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = self.lib.heap_emu_distances(p(parent), p(dist), ctypes.c_int64(len(parent)), p(pairs), ctypes.c_int64(len(pairs)), p(d), p(m))
        assert rc == 0, self.lib.heap_emu_last_error().decode()
        return d, m


@pytest.fixture(scope="module")
def heap_emu():
    return HeapEmulator()


def mixed_leaf_pairs(levels, seed, n_random=300_000, n_near=100_000, n_same=100_000):
    """Random leaf pairs, pairs within +-70 leaves of each other, and pairs with a == b (node ids)."""
    rng = np.random.default_rng(seed)
    leaves = 1 << levels
    rand = rng.integers(0, leaves, (n_random, 2))
    a = rng.integers(0, leaves, n_near)
    near = np.stack([a, np.clip(a + rng.integers(-70, 71, n_near), 0, leaves - 1)], axis=1)
    same = np.repeat(rng.integers(0, leaves, n_same)[:, None], 2, axis=1)
    return (np.concatenate([rand, near, same]) * 2).astype(np.int64)


def _check(heap_emu, parent, dist, pairs):
    want_d, want_m = oracle_both(parent, dist, pairs)
    d, m = heap_emu.run(parent, dist, pairs)
    assert_bits_equal(d, want_d)
    assert np.array_equal(m, want_m)


@pytest.mark.parametrize("levels", [6, 7, 10, 16, 20])
def test_perfect_trees_are_admitted_with_the_stated_table_sizes(heap_emu, levels):
    ok, n_lines, n_heap, got_levels = heap_emu.prepare(*synth.balanced_tree(levels))
    assert ok and got_levels == levels
    assert n_lines == 32 * 2 ** (levels - 4) and n_heap == 2 ** (levels - 5)


def test_other_trees_are_refused_and_leave_no_tables(heap_emu):
    swapped_p, swapped_d = synth.balanced_tree(8)
    swapped_p = swapped_p.copy()
    # two parents swapped: leaves 0 and 4 trade places (ids 1 and 5 are their parents) -- still a binary tree with every leaf
    # at depth 8 and the leaves on the even ids, but not the in-order shape
    swapped_p[0], swapped_p[4] = swapped_p[4], swapped_p[0]
    for name, (parent, dist) in (("5 levels", synth.balanced_tree(5)), ("21 levels", synth.balanced_tree(21)),
                                 ("complete", synth.complete_tree(50_000)), ("random", synth.random_binary_tree(4096)),
                                 ("swapped", (swapped_p, swapped_d))):
        assert heap_emu.prepare(parent, dist) == (False, 0, 0, 0), name


def test_every_leaf_pair_of_64_leaves(heap_emu):
    parent, dist = synth.balanced_tree(6)
    a, b = np.meshgrid(np.arange(64) * 2, np.arange(64) * 2, indexing="ij")
    _check(heap_emu, parent, dist, np.stack([a.ravel(), b.ravel()], axis=1))


@pytest.mark.parametrize("levels", [7, 10, 16])
def test_random_near_and_equal_leaf_pairs(heap_emu, levels):
    parent, dist = synth.balanced_tree(levels)
    _check(heap_emu, parent, dist, mixed_leaf_pairs(levels, seed=levels))


def test_internal_nodes_take_the_walk(heap_emu):
    parent, dist = synth.balanced_tree(7)
    n = len(parent)
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    _check(heap_emu, parent, dist, np.stack([a.ravel(), b.ravel()], axis=1))


def test_special_float_values(heap_emu):
    """Denormals, signed zeros, huge and negative lengths must add exactly as on the CPU (the mix of
    test_tables_emulated.py::test_special_float_values, planted into a perfect tree)."""
    parent, dist = synth.balanced_tree(11)
    rng = np.random.default_rng(4)
    dist = dist.copy()
    k = rng.integers(0, len(dist), 600)
    dist[k[:100]] = np.float32(1e-42)       # denormal
    dist[k[100:200]] = np.float32(-0.0)
    dist[k[200:300]] = np.float32(3e38)
    dist[k[300:400]] = np.float32(-1.5)
    dist[k[400:500]] = np.float32(2.220446e-16)
    dist[k[500:]] = np.float32(1.17549435e-38)
    _check(heap_emu, parent, dist, mixed_leaf_pairs(11, seed=4))
    # ... and where every edge is -0.0: sums start at +0.0, so every distance is +0.0 as the reference's is
    zeros = np.full(len(dist), np.float32(-0.0), np.float32)
    _check(heap_emu, parent, zeros, mixed_leaf_pairs(11, seed=5, n_random=20_000, n_near=5_000, n_same=1_000))
