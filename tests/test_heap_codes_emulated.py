"""Heap codes of perfect trees (tree_prep.cpp: prepare_heap_codes; tree_prep.h: the place, extraction and decoding functions
of k_canopy_ilp_codes) on the CPU (tests/emu/heap_codes_emulator.cpp, compiled with g++ over the same functions): the decoder
over all 2^20 codes, the table of 6- to 9-level trees leaf slot by leaf slot, the extreme codes, the trees that must be
refused, and the kernel's pair function against the oracle, by bits: every node pair of small trees, uniform pairs of 2^14
leaves, and at 8, 13, 19 and 20 levels every k (tests/heap_pair_cases.py: by_k_pairs, grouped and shuffled) and the slots at the
edges of the code lines (edge_slot_pairs) -- the index arithmetic of tests/emu/heap_pair_emu.h and tree_prep.h at depth."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, oracle_both
from heap_pair_cases import by_k_pairs, edge_slot_pairs, oracle_answers
from oracle.oracle import OracleTree
from suchtree_amd import synth

PAD_WORDS = 4      # tree_prep.h: kHeapCodePadWords


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class CodesEmulator:
    def __init__(self):
        emu_dir = os.path.join(ROOT, "tests", "emu")
        lib = os.path.join(emu_dir, "libst_heap_codes_emu.so")
        srcs = [os.path.join(emu_dir, "heap_codes_emulator.cpp"), os.path.join(ROOT, "suchtree_amd", "csrc", "tree_prep.cpp")]
        deps = srcs + [os.path.join(ROOT, "suchtree_amd", "csrc", h) for h in ("tree_prep.h", "pair_math.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            tmp = "%s.tmp.%d" % (lib, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + srcs)
            os.replace(tmp, lib)
        self.lib = ctypes.CDLL(lib)
        self.lib.codes_emu_last_error.restype = ctypes.c_char_p
        self.lib.codes_emu_code_of.argtypes = [ctypes.c_float, ctypes.c_void_p]
        self.lib.codes_emu_lane_pairs.restype = ctypes.c_int64

    def error(self):
        return self.lib.codes_emu_last_error().decode()

    def decode(self, codes, f32):
        codes = np.ascontiguousarray(codes, np.uint32)
        out = np.zeros(len(codes), np.float32)
        self.lib.codes_emu_decode(_p(codes), ctypes.c_int64(len(codes)), ctypes.c_int(1 if f32 else 0), _p(out))
        return out

    def code_of(self, x):
        c = np.zeros(1, np.uint32)
        return int(c[0]) if self.lib.codes_emu_code_of(ctypes.c_float(float(np.float32(x))), _p(c)) else None

    def prepare(self, parent, dist):
        """(return code, floats of heap_lines, words of heap_codes, levels, the table)"""
        parent, dist = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(dist, np.float32)
        sizes = np.zeros(3, np.int64)
        words = np.full(len(parent) + 64, 0xFFFFFFFF, np.uint32)      # (20 bits per edge and two copies: always room)
        rc = self.lib.codes_emu_prepare(_p(parent), _p(dist), ctypes.c_int64(len(parent)), _p(sizes), _p(words), ctypes.c_int64(len(words)))
        assert rc in (0, 2, 3), self.error()
        return rc, int(sizes[0]), int(sizes[1]), int(sizes[2]), words[:int(sizes[1])].copy()

    def lineage(self, table, n_words, slot):
        out = np.zeros(6, np.float32)
        rc = self.lib.codes_emu_lineage(_p(table), ctypes.c_int64(n_words), ctypes.c_uint32(slot), _p(out))
        return rc, out

    def run(self, parent, dist, pairs):
        parent, dist = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(dist, np.float32)
        pairs = np.ascontiguousarray(pairs, np.int64)
        d, m = np.zeros(len(pairs)), np.zeros(len(pairs), np.int32)
        rc = self.lib.codes_emu_distances(_p(parent), _p(dist), ctypes.c_int64(len(parent)), _p(pairs), ctypes.c_int64(len(pairs)), _p(d), _p(m))
        assert rc == 0, self.error()
        return d, m


@pytest.fixture(scope="module")
def emu():
    return CodesEmulator()


def _lines(levels):
    return -(-(1 << (levels - 3)) // 3)


def _lineage_of(parent, dist, slot):
    """The six lowest edges above leaf slot `slot`, from the tree's own arrays."""
    x, out = 2 * slot, []
    for _ in range(6):
        out.append(dist[x])
        x = parent[x]
    return np.asarray(out, np.float32)


def _check_table(emu, parent, dist, levels):
    rc, n_lines, n_words, got_levels, table = emu.prepare(parent, dist)
    assert rc == 0 and got_levels == levels
    assert n_lines == 32 * 2 ** (levels - 4) and n_words == 32 * _lines(levels) + PAD_WORDS
    assert not table[32 * _lines(levels):].any()      # the padding is zero
    for slot in range(1 << levels):
        # (the emulated loads are refused beyond 32 words per line: the padding is not there to be read)
        rc, got = emu.lineage(table, n_words - PAD_WORDS, slot)
        assert rc == 0, emu.error()
        assert np.array_equal(got.view(np.uint32), _lineage_of(parent, dist, slot).view(np.uint32)), (levels, slot)
    return table


def test_decoder_is_float32_of_c_over_1e6_for_every_code(emu):
    codes = np.arange(1 << 20, dtype=np.uint32)
    want = (codes.astype(np.float64) / 1e6).astype(np.float32)
    assert np.array_equal(emu.decode(codes, f32=False).view(np.uint32), want.view(np.uint32))
    # the kernel's form: four float32 operations with a real fmaf
    assert np.array_equal(emu.decode(codes, f32=True).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("levels", [6, 7, 8, 9])
def test_every_leaf_slot_finds_its_six_edges(emu, levels):
    """The last line holds 2, 1, 2 and 1 subtrees at these sizes; its unused fields are zero."""
    parent, dist = synth.balanced_tree(levels)
    table = _check_table(emu, parent, dist, levels)
    used = (1 << (levels - 3)) - 3 * (_lines(levels) - 1)
    assert used == {6: 2, 7: 1, 8: 2, 9: 1}[levels]
    last = table[32 * (_lines(levels) - 1):32 * _lines(levels)]
    bits = np.unpackbits(last.view(np.uint8), bitorder="little")
    assert not bits[340 * used:].any() and bits[:340 * used].any()


@pytest.mark.parametrize("levels", [6, 7])
def test_lanes_l_and_l_xor_1_share_their_loads(emu, levels):
    """Every slot on the even lane with every slot on the odd lane: each lane ends up with the six codes it finds on its own,
    and either step's two loads fall on one line -- over the tree's table and over one of random bits."""
    parent, dist = synth.balanced_tree(levels)
    _, _, n_words, _, table = emu.prepare(parent, dist)
    noise = np.random.default_rng(levels).integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32)
    for what, words in (("tree", table), ("random bits", noise)):
        bad = emu.lib.codes_emu_lane_pairs(_p(words), ctypes.c_int64(n_words - PAD_WORDS), ctypes.c_uint32(1 << levels))
        assert bad == 0, (what, bad, emu.error())


def test_every_benchmark_edge_has_a_code_and_most_random_lengths_have_none(emu):
    for levels in (6, 7, 12):
        _, dist = synth.balanced_tree(levels)
        root = (1 << levels) - 1
        codes = [emu.code_of(x) for k, x in enumerate(dist) if k != root]
        assert None not in codes and max(codes) <= 1_000_000
    # lengths that were never rounded: a few are six-decimal numbers by chance, most are not -- one is enough to refuse a tree
    parent, dist = synth.random_binary_tree(64)
    without = sum(emu.code_of(x) is None for k, x in enumerate(dist) if parent[k] >= 0)
    assert without > 100, without


def test_extreme_codes(emu):
    """Code 0 (+0.0f) and code 1,048,575 on every level the table holds, and beside each other."""
    levels = 7
    parent, dist = synth.balanced_tree(levels)
    dist = dist.copy()
    top, zero = np.float32(1048575 / 1e6), np.float32(0.0)
    assert emu.code_of(top) == 1048575 and emu.code_of(zero) == 0
    for h in range(6):      # node (h, k) has id (2k+1) * 2^h - 1
        count = 1 << (levels - h)
        for k in range(count):
            if k % 3 == 0:
                dist[(2 * k + 1) * (1 << h) - 1] = top if (k // 3 + h) % 2 == 0 else zero
    _check_table(emu, parent, dist, levels)
    every = np.full(len(dist), top, np.float32)
    table = _check_table(emu, parent, every, levels)
    assert (np.unpackbits(table[:32].view(np.uint8), bitorder="little")[:1020] == 1).all()
    _check_table(emu, parent, np.zeros(len(dist), np.float32), levels)


@pytest.mark.parametrize("value", [np.float32(1.048576), np.float32(0.1234567), np.float32(-0.0), np.finfo(np.float32).eps])
@pytest.mark.parametrize("node", [0, 1, 31, 126])      # a leaf, its parent, a level-5 edge, the last leaf of the last line
def test_one_edge_without_a_code_refuses_the_table_and_keeps_the_heap_lines(emu, value, node):
    parent, dist = synth.balanced_tree(6)
    dist = dist.copy()
    dist[node] = value
    assert emu.code_of(value) is None
    rc, n_lines, n_words, levels, _ = emu.prepare(parent, dist)
    assert rc == 3 and n_lines == 32 * 4 and n_words == 0 and levels == 6


def test_trees_without_heap_lines_get_no_codes(emu):
    for parent, dist in (synth.balanced_tree(5), synth.random_binary_tree(64)):
        rc, n_lines, n_words, _, _ = emu.prepare(parent, dist)
        assert rc == 2 and n_lines == 0 and n_words == 0


def test_a_load_past_the_table_is_noticed(emu):
    """(the emulator's own bound check: a slot beyond the table must not read)"""
    parent, dist = synth.balanced_tree(6)
    _, _, n_words, _, table = emu.prepare(parent, dist)
    rc, _ = emu.lineage(table, n_words, 1 << 7)
    assert rc == 1 and "past the table" in emu.error()


@pytest.mark.parametrize("levels", [6, 7])
def test_every_node_pair_against_the_oracle(emu, levels):
    parent, dist = synth.balanced_tree(levels)
    n = len(parent)
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pairs = np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int64)
    want_d, want_m = oracle_both(parent, dist, pairs)
    d, m = emu.run(parent, dist, pairs)
    assert_bits_equal(d, want_d)
    assert np.array_equal(m, want_m)


def test_random_leaf_pairs_of_2_14_leaves_against_the_oracle(emu):
    levels = 14
    parent, dist = synth.balanced_tree(levels)
    pairs = synth.random_leaf_pairs(1 << levels, 200_000, seed=14)
    want_d, want_m = oracle_both(parent, dist, pairs)
    d, m = emu.run(parent, dist, pairs)
    assert_bits_equal(d, want_d)
    assert np.array_equal(m, want_m)


@pytest.mark.parametrize("levels", [8, 13, 19, 20])
def test_every_k_and_the_edge_slots_at_depth_against_the_oracle(emu, levels):
    """The climb through the heap image has levels - 6 terms per side: 2, 7, 13 and 14 here (uniform pairs of a deep tree
    take nearly all of them nearly always: by_k_pairs stops after each number of them equally often)."""
    parent, dist = synth.balanced_tree(levels)
    grouped, shuffled = by_k_pairs(levels, 2048, seed=100 + levels)
    batches = (("every k, grouped", grouped), ("every k, shuffled", shuffled), ("edge slots", edge_slot_pairs(levels, seed=200 + levels)))
    pairs = np.concatenate([b for _, b in batches])
    want_d, want_m = oracle_answers(OracleTree(parent, dist), pairs)
    d, m = emu.run(parent, dist, pairs)      # (one call: the emulator prepares the tree's tables in every call)
    lo = 0
    for what, b in batches:
        hi = lo + len(b)
        assert_bits_equal(d[lo:hi], want_d[lo:hi], "%d levels, %s" % (levels, what))
        assert np.array_equal(m[lo:hi], want_m[lo:hi]), (levels, what)
        lo = hi
    x = (grouped[:, 0] >> 1) ^ (grouped[:, 1] >> 1)
    assert int(x.max()).bit_length() == levels and np.count_nonzero(x == 0) == 2048      # k from 0 to the root
