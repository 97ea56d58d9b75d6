"""The heap-line form of the predicated kernel (k_canopy_ilp_heap; perfect trees) on the GPU against the oracle, by bits:
every node pair and every leaf pair of small trees, random / near / equal / internal pairs of a 2^16-leaf tree, tail tiles,
every sink, and the default handle of a 2^18-leaf tree.  Batches have at least 4096 pairs (smaller ones go to the walk
family and never reach the kernel)."""
import numpy as np
import pytest

from conftest import assert_bits_equal, oracle_both
from suchtree_amd import _capi, sharding, synth
from suchtree_amd.exceptions import InvalidNodeError

pytestmark = pytest.mark.gpu

MIN_BATCH = 4096


def _tile(pairs, least=MIN_BATCH):
    reps = -(-least // len(pairs))
    return np.ascontiguousarray(np.tile(pairs, (reps, 1)), np.int64)


def _all_pairs(ids):
    a, b = np.meshgrid(ids, ids, indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int64)


def _heap_tree(levels):
    parent, dist = synth.balanced_tree(levels)
    dev = _capi.DeviceTree(parent, dist)
    dev.set_option("heap_lines", 2)
    info = dev.info()
    assert info["heap_lines"] == 1 and info["big_batch_kernel"] == "canopy", info
    assert (info["a_side_bytes"], info["b_table_bytes_per_leaf"]) == (4, 4), info
    return parent, dist, dev


def _check_every_sink(dev, pairs, want_d, want_m, what):
    """int64 device buffers (float64 sink), int32 ids through the host path, and the float32 and packed wire sinks against the
    same handle without the form."""
    import torch
    n = len(pairs)
    assert n >= MIN_BATCH
    t = torch.from_numpy(pairs).cuda()
    out_d = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    out_m = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
    dev.fault_check()
    assert_bits_equal(out_d.cpu().numpy(), want_d, what + ": int64 device buffers")
    assert np.array_equal(out_m.cpu().numpy(), want_m), what
    d, m = dev.distances_host(pairs.astype(np.int32), True, True)
    assert_bits_equal(d, want_d, what + ": int32 host path")
    assert np.array_equal(m, want_m), what
    got = {}
    for heap in (0, 2):
        dev.set_option("heap_lines", heap)
        assert dev.info()["heap_lines"] == (1 if heap else 0)
        f32_d = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        f32_m = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        dev.distances_device(t.data_ptr(), n, f32_d.data_ptr(), f32_m.data_ptr(), f32=True)
        wire_d = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        wire_m = torch.full((sharding.packed_bytes(n) + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        dev.distances_device_wire(t.data_ptr(), n, wire_d.data_ptr(), wire_m.data_ptr())
        dev.fault_check()
        assert bool((wire_m[sharding.packed_bytes(n):] == 0xEE).all()), what      # nothing written past the last dword
        unpacked = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        dev.unpack_mrca24_device(wire_m.data_ptr(), n, unpacked.data_ptr())
        got[heap] = [x.cpu().numpy() for x in (f32_d, f32_m, wire_d, unpacked)]
    for with_form, without in zip(got[2], got[0]):
        assert np.array_equal(with_form.view(np.int32), without.view(np.int32)), what
    assert_bits_equal(got[2][0].astype(np.float64), want_d, what + ": float32 sink")
    assert np.array_equal(got[2][3], want_m), what


@pytest.mark.parametrize("levels", [6, 7])
def test_every_node_pair_and_every_leaf_pair_of_small_trees(levels):
    parent, dist, dev = _heap_tree(levels)
    n = len(parent)
    for what, pairs in (("node pairs", _tile(_all_pairs(np.arange(n)))), ("leaf pairs", _tile(_all_pairs(np.arange(0, n, 2))))):
        want_d, want_m = oracle_both(parent, dist, pairs)
        _check_every_sink(dev, pairs, want_d, want_m, "%d levels, %s" % (levels, what))
    dev.close()


@pytest.fixture(scope="module")
def levels16():
    """2^16 leaves: 2e5 random leaf pairs, 1e5 near pairs (+-70 leaves), a == b, a mix of internal ids; the oracle once."""
    levels = 16
    parent, dist, dev = _heap_tree(levels)
    rng = np.random.default_rng(16)
    leaves, n = 1 << levels, len(parent)
    rand = rng.integers(0, leaves, (200_000, 2)) * 2
    a = rng.integers(0, leaves, 100_000)
    near = np.stack([a, np.clip(a + rng.integers(-70, 71, len(a)), 0, leaves - 1)], axis=1) * 2
    same = np.repeat(rng.integers(0, leaves, 20_000)[:, None], 2, axis=1) * 2
    internal = rng.integers(0, n, (30_000, 2))
    internal[::3, 0] = rng.integers(0, leaves, len(internal[::3])) * 2      # (leaf with internal node, both orders, node with itself)
    internal[1::7, 1] = internal[1::7, 0]
    pairs = np.concatenate([rand, near, same, internal]).astype(np.int64)
    pairs = pairs[rng.permutation(len(pairs))]
    want_d, want_m = oracle_both(parent, dist, pairs)
    want_d.setflags(write=False)
    want_m.setflags(write=False)
    yield dev, pairs, want_d, want_m
    dev.close()


def test_random_near_equal_and_internal_pairs_of_2_16_leaves(levels16):
    dev, pairs, want_d, want_m = levels16
    _check_every_sink(dev, pairs, want_d, want_m, "16 levels")


@pytest.mark.parametrize("n", [MIN_BATCH + 1, MIN_BATCH + 63, MIN_BATCH + 1025])
def test_tail_tiles(levels16, n):
    dev, pairs, want_d, want_m = levels16
    _check_every_sink(dev, np.ascontiguousarray(pairs[:n]), want_d[:n], want_m[:n], "16 levels, %d pairs" % n)


def test_out_of_range_ids_are_reported(levels16):
    """Fault record, NaN and -1, exactly as the other canopy kernels answer."""
    import torch
    dev, pairs, want_d, want_m = levels16
    n = 8192
    bad = pairs[:n].copy()
    bad[5, 0], bad[4097, 1] = -3, 1 << 40
    t = torch.from_numpy(bad).cuda()
    out_d = torch.zeros(n, dtype=torch.float64, device="cuda")
    out_m = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
    with pytest.raises(InvalidNodeError):
        dev.fault_check()
    d, m = out_d.cpu().numpy(), out_m.cpu().numpy()
    ok = np.ones(n, bool)
    ok[[5, 4097]] = False
    assert np.isnan(d[~ok]).all() and (m[~ok] == -1).all()
    assert_bits_equal(d[ok], want_d[:n][ok])
    assert np.array_equal(m[ok], want_m[:n][ok])


def test_default_handle_of_2_18_leaves_takes_the_form():
    import torch
    levels = 18
    parent, dist = synth.balanced_tree(levels)
    dev = _capi.DeviceTree(parent, dist)
    info = dev.info()
    assert info["heap_lines"] == 1 and info["b_table_bytes_per_leaf"] == 4 and info["a_side_bytes"] == 4, info
    assert info["big_batch_kernel"] == "canopy", info
    pairs = synth.random_leaf_pairs(1 << levels, 1_000_000, seed=18)
    want_d, want_m = oracle_both(parent, dist, pairs)
    t = torch.from_numpy(pairs).cuda()
    out_d = torch.empty(len(pairs), dtype=torch.float64, device="cuda")
    out_m = torch.empty(len(pairs), dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), len(pairs), out_d.data_ptr(), out_m.data_ptr())
    dev.fault_check()
    with_d, with_m = out_d.cpu().numpy(), out_m.cpu().numpy()
    assert_bits_equal(with_d, want_d, "default handle")
    assert np.array_equal(with_m, want_m)
    dev.set_option("heap_lines", 0)
    info = dev.info()
    assert info["heap_lines"] == 0 and info["b_table_bytes_per_leaf"] == info["record_bytes"] // 4, info
    out_d.fill_(-7.0)
    out_m.fill_(-9)
    dev.distances_device(t.data_ptr(), len(pairs), out_d.data_ptr(), out_m.data_ptr())
    dev.fault_check()
    assert_bits_equal(out_d.cpu().numpy(), with_d, "heap_lines = 0")
    assert np.array_equal(out_m.cpu().numpy(), with_m)
    dev.close()
    # a 2^16-leaf tree keeps the tables it had by default
    small = _capi.DeviceTree(*synth.balanced_tree(16))
    assert small.info()["heap_lines"] == 0 and small.info()["b_table_bytes_per_leaf"] == 8
    small.close()
