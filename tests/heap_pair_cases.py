"""Shared inputs and checks of the heap-code tests (tests/test_gpu_heap_codes.py, tests/test_gpu_heap_codes_depth.py,
tests/test_heap_codes_emulated.py): leaf-pair batches of perfect trees in which every number of edges k between a leaf and
the pair's MRCA occurs equally often (uniform pairs of 2^20 leaves have k = 19 or 20 three times in four), batches around the
slots at which a 128-byte line of codes begins and ends, the mixed batch with internal nodes and equal ids, the oracle's
answers from one OracleTree, and the device sinks between canaries.  The generators are plain numpy."""
import os

import numpy as np

from conftest import assert_bits_equal
from suchtree_amd import sharding

MIN_BATCH = 4096      # smaller batches go to the walk family and never reach the heap kernels
CODE_LINE_SLOTS = 24      # leaf slots that share one 128-byte line of 20-bit codes (tree_prep.h)


def by_k_pairs(levels, per_k, seed):
    """(grouped, shuffled): for every k in 0 .. levels, per_k leaf pairs of a perfect tree of `levels` levels whose slots
    part exactly k edges below their MRCA -- sa uniform, sb = sa for k = 0, else sa ^ (2^(k-1) | r) with r uniform below
    2^(k-1); ids are 2 * slot.  grouped: k = 0 first, so that k is the same over a wave; shuffled: the same pairs in a seeded
    random order."""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(levels + 1):
        sa = rng.integers(0, 1 << levels, per_k, dtype=np.int64)
        if k == 0:
            sb = sa.copy()
        else:
            sb = sa ^ ((1 << (k - 1)) | rng.integers(0, 1 << (k - 1), per_k, dtype=np.int64))
        parts.append(np.stack([sa, sb], axis=1))
    slots = np.concatenate(parts)
    assert slots.min() >= 0 and slots.max() < 1 << levels
    x = slots[:, 0] ^ slots[:, 1]
    k_of = np.where(x == 0, 0, np.floor(np.log2(np.maximum(x, 1))).astype(np.int64) + 1)
    assert np.array_equal(np.bincount(k_of, minlength=levels + 1), np.full(levels + 1, per_k)), "every k occurs per_k times"
    assert np.array_equal(k_of, np.repeat(np.arange(levels + 1), per_k))
    grouped = np.ascontiguousarray(2 * slots, np.int64)
    shuffled = np.ascontiguousarray(grouped[rng.permutation(len(grouped))])
    return grouped, shuffled


def edge_slots(levels):
    """The slots at the edges of the lines: the first ones, those around the first line boundaries of the float lines (16 slots)
    and of the code lines (24 slots), those around the code line boundary in the middle of the tree, and the last 50 slots,
    which reach the last code line (it holds 1 or 2 of its 3 groups of 8) and the line before it."""
    leaves = 1 << levels
    mid = CODE_LINE_SLOTS * (leaves // (2 * CODE_LINE_SLOTS))
    e = [0, 1, 15, 16, 23, 24, 47, 48, 63, 64, 65, mid - 1, mid, mid + 1] + list(range(leaves - 50, leaves))
    return np.unique(np.clip(np.asarray(e, dtype=np.int64), 0, leaves - 1))


def edge_slot_pairs(levels, seed):
    """Every ordered pair of edge_slots(levels), every edge slot against 256 random slots in both orders, random leaf pairs up
    to at least MIN_BATCH + 63 pairs; shuffled.  Ids are 2 * slot."""
    rng = np.random.default_rng(seed)
    leaves = 1 << levels
    e = edge_slots(levels)
    a, b = np.meshgrid(e, e, indexing="ij")
    parts = [np.stack([a.ravel(), b.ravel()], axis=1)]
    other = rng.integers(0, leaves, (len(e), 256), dtype=np.int64)
    own = np.broadcast_to(e[:, None], other.shape)
    parts += [np.stack([own.ravel(), other.ravel()], axis=1), np.stack([other.ravel(), own.ravel()], axis=1)]
    have = sum(len(p) for p in parts)
    parts.append(rng.integers(0, leaves, (max(MIN_BATCH + 63 - have, 64), 2), dtype=np.int64))
    slots = np.concatenate(parts)
    assert len(slots) >= MIN_BATCH + 63 and slots.min() >= 0 and slots.max() < leaves
    return np.ascontiguousarray(2 * slots[rng.permutation(len(slots))], np.int64)


def oracle_answers(tree, pairs, threads=None):
    """(distances, MRCA ids) of ONE OracleTree on all host cores (a tree of 2^20 leaves takes seconds to build: the threads
    of conftest.oracle_both build one each).  The C calls release the GIL and every call has its own visited list.  Read-only."""
    from concurrent.futures import ThreadPoolExecutor
    pairs = np.ascontiguousarray(pairs, np.int64)
    n = len(pairs)
    k = max(1, min(threads or min(32, len(os.sched_getaffinity(0))), n // 256))
    d = tree.distances_mt(pairs, k)
    bounds = [n * i // k for i in range(k + 1)]
    with ThreadPoolExecutor(k) as ex:
        parts = list(ex.map(lambda i: tree.mrca_bulk(pairs[bounds[i]:bounds[i + 1]]), range(k)))
    m = np.concatenate(parts)
    d.setflags(write=False)
    m.setflags(write=False)
    return d, m


def _mixed_pairs(n_nodes, n, seed):
    """Leaf pairs, pairs with internal nodes, equal ids and neighbours, shuffled."""
    rng = np.random.default_rng(seed)
    leaves = (n_nodes + 1) // 2
    q = n // 4
    rand = rng.integers(0, leaves, (n - 3 * q, 2)) * 2
    internal = rng.integers(0, n_nodes, (q, 2))
    internal[::3, 0] = rng.integers(0, leaves, len(internal[::3])) * 2
    same = np.repeat(rng.integers(0, n_nodes, q)[:, None], 2, axis=1)
    a = rng.integers(0, leaves, q)
    near = np.stack([a, np.clip(a + rng.integers(-3, 4, q), 0, leaves - 1)], axis=1) * 2
    pairs = np.concatenate([rand, internal, same, near]).astype(np.int64)
    return np.ascontiguousarray(pairs[rng.permutation(len(pairs))])


def _device_sinks(dev, t_pairs, n):
    """float64 + int32, float32 + int32 and the wire form (float32 + packed ids) for the first n pairs, between canaries."""
    import torch
    ptr = t_pairs.data_ptr()
    pb = sharding.packed_bytes(n)
    d64 = torch.full((n + 8,), -7.0, dtype=torch.float64, device="cuda")
    m_a = torch.full((n + 8,), -9, dtype=torch.int32, device="cuda")
    dev.distances_device(ptr, n, d64.data_ptr() + 4 * 8, m_a.data_ptr() + 4 * 4)
    f32 = torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")
    m_b = torch.full((n + 8,), -9, dtype=torch.int32, device="cuda")
    dev.distances_device(ptr, n, f32.data_ptr() + 4 * 4, m_b.data_ptr() + 4 * 4, f32=True)
    w32 = torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")
    m24 = torch.full((16 + pb + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    dev.distances_device_wire(ptr, n, w32.data_ptr() + 4 * 4, m24.data_ptr() + 16)
    m_c = torch.full((n + 8,), -9, dtype=torch.int32, device="cuda")
    dev.unpack_mrca24_device(m24.data_ptr() + 16, n, m_c.data_ptr() + 4 * 4)
    dev.fault_check()
    for buf, canary in ((d64, -7.0), (f32, -7.0), (w32, -7.0), (m_a, -9), (m_b, -9), (m_c, -9)):
        assert bool((buf[:4] == canary).all()) and bool((buf[n + 4:] == canary).all()), "a store outside [0, n)"
    assert bool((m24[:16] == 0xEE).all()) and bool((m24[16 + pb:] == 0xEE).all()), "a store outside the packed ids"
    return [x[4:n + 4].cpu().numpy() for x in (d64, m_a, f32, m_b, w32, m_c)]


def _check_against_oracle(got, want_d, want_m, what):
    d64, m_a, f32, m_b, w32, m_c = got
    assert_bits_equal(d64, want_d, what + ": float64 sink")
    assert_bits_equal(f32.astype(np.float64), want_d, what + ": float32 sink")
    assert_bits_equal(w32.astype(np.float64), want_d, what + ": wire sink")
    for m in (m_a, m_b, m_c):
        assert np.array_equal(m, want_m), what
