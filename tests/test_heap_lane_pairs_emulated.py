"""The shared line loads of k_canopy_ilp_heap's lane pairs on the CPU (tests/emu/lane_pairs_emulator.cpp, compiled with g++
over the offset functions the kernel uses: tree_prep.h, heap_pair_offset): lanes l and l ^ 1 read the window of one slot and
the top of the same slot in one step, swap, and every lane must end up with exactly the eight floats it read on its own before
-- the 16-byte window of its slot and the last four floats of its line."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from suchtree_amd import synth

LEVELS = 7      # 128 leaf slots, 8 lines


class LanePairs:
    def __init__(self):
        emu_dir = os.path.join(ROOT, "tests", "emu")
        lib = os.path.join(emu_dir, "libst_lane_pairs_emu.so")
        srcs = [os.path.join(emu_dir, "lane_pairs_emulator.cpp"), os.path.join(ROOT, "suchtree_amd", "csrc", "tree_prep.cpp")]
        deps = srcs + [os.path.join(ROOT, "suchtree_amd", "csrc", "tree_prep.h")]
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            tmp = "%s.tmp.%d" % (lib, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + srcs)
            os.replace(tmp, lib)
        self.lib = ctypes.CDLL(lib)
        self.lib.lane_pairs_last_error.restype = ctypes.c_char_p
        self.lib.lane_pairs_table.restype = ctypes.c_int64
        self.lib.lane_pairs_sweep.restype = ctypes.c_int64

    def error(self):
        return self.lib.lane_pairs_last_error().decode()

    def table(self, levels):
        parent, dist = synth.balanced_tree(levels)
        parent, dist = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(dist, np.float32)
        out = np.zeros(32 << (levels - 4), np.float32)
        n = self.lib.lane_pairs_table(parent.ctypes.data_as(ctypes.c_void_p), dist.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.c_int64(len(parent)), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(out)))
        assert n == len(out), self.error()
        return out

    def offsets(self, slot):
        out = (ctypes.c_uint32 * 2)()
        self.lib.lane_pairs_offsets(ctypes.c_uint32(slot), out)
        return out[0], out[1]

    def quad(self, lines, slots):
        out, touched = np.zeros(32, np.float32), np.zeros(2, np.int32)
        q = np.asarray(slots, np.uint32)
        rc = self.lib.lane_pairs_quad(lines.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(lines)), q.ctypes.data_as(ctypes.c_void_p),
                                      out.ctypes.data_as(ctypes.c_void_p), touched.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, self.error()
        return out.reshape(4, 8), touched

    def sweep(self, lines, n_slots):
        return self.lib.lane_pairs_sweep(lines.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(lines)), ctypes.c_uint32(n_slots))


@pytest.fixture(scope="module")
def lane_pairs():
    return LanePairs()


def _alone(lines, slot):
    """What a lane read on its own: floats 7g .. 7g+3 or 7g+3 .. 7g+6 of its line (tree_prep.h), then floats 28 .. 31."""
    line, t = 32 * (slot >> 4), slot & 15
    w = line + 7 * (t >> 2) + (3 if t & 2 else 0)
    return np.concatenate([lines[w:w + 4], lines[line + 28:line + 32]])


def test_offsets_are_the_layout_of_a_heap_line(lane_pairs):
    for slot in (0, 1, 2, 3, 4, 7, 13, 15, 16, 18, 127, (1 << 19) - 1):
        line, t = 32 * (slot >> 4), slot & 15
        assert lane_pairs.offsets(slot) == (line + 7 * (t >> 2) + (3 if t & 2 else 0), line + 28), slot
    # step 0 serves the even lane's slot (it reads its window, the odd lane that slot's top), step 1 the odd lane's
    assert [[lane_pairs.lib.lane_pairs_reads_window(step, lane) for lane in range(4)] for step in (0, 1)] == [[1, 0, 1, 0], [0, 1, 0, 1]]


def test_every_slot_parity_and_neighbour_slot_of_128_leaves(lane_pairs):
    """Own slot x neighbour slot, the own slot on an even and on an odd lane of the quad: 16384 quads over the tree's own table
    and over one whose every float names its position."""
    for what, lines in (("tree", lane_pairs.table(LEVELS)), ("positions", np.arange(32 << (LEVELS - 4), dtype=np.float32))):
        assert lane_pairs.sweep(lines, 1 << LEVELS) == 0, (what, lane_pairs.error())


def test_a_quad_lane_by_lane(lane_pairs):
    """The same through Python for a few quads of four different slots: each lane's eight floats, and per step two lines, each
    read by two adjacent lanes."""
    lines = np.arange(32 << (LEVELS - 4), dtype=np.float32)
    rng = np.random.default_rng(7)
    quads = [(0, 17, 34, 51), (127, 0, 5, 5), (3, 2, 1, 0), (15, 16, 31, 32)] + [tuple(q) for q in rng.integers(0, 1 << LEVELS, (60, 4))]
    for q in quads:
        got, touched = lane_pairs.quad(lines, q)
        for lane in range(4):
            assert np.array_equal(got[lane], _alone(lines, int(q[lane]))), (q, lane)
        for step in (0, 1):
            served = {q[step] >> 4, q[2 + step] >> 4}      # the lines of the slots that step serves (lanes 0, 2 / 1, 3)
            assert touched[step] == len(served), (q, step)


def test_a_load_past_the_table_is_noticed(lane_pairs):
    """(the emulator's own bound check: a slot beyond the table must not read)"""
    lines = np.zeros(32 << (LEVELS - 4), np.float32)
    out, touched = np.zeros(32, np.float32), np.zeros(2, np.int32)
    q = np.asarray([0, 1 << LEVELS, 0, 0], np.uint32)
    rc = lane_pairs.lib.lane_pairs_quad(lines.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(lines)), q.ctypes.data_as(ctypes.c_void_p),
                                        out.ctypes.data_as(ctypes.c_void_p), touched.ctypes.data_as(ctypes.c_void_p))
    assert rc == 1 and "past the table" in lane_pairs.error()
