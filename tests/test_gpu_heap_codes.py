"""The heap-code form of the predicated kernel (k_canopy_ilp_codes; perfect trees whose edges are six-decimal numbers) on the GPU
against the oracle, by bits: every leaf pair of 6- and 7-level trees in order and shifted by one position (each pair on an even
and on an odd lane), every sink, both pair sources, with and without the streaming hint, tail tiles, internal nodes, equal ids
and ids out of range beside leaf pairs, the form against the heap lines on the same handle, a tree that is refused, and what a
default handle reports.  Batches have at least 4096 pairs (smaller ones go to the walk family and never reach the kernel).  The mixed
batch and the sinks between canaries are those of tests/heap_pair_cases.py; deeper trees, every k, more pairs than one trip of the
grid and the default policy are in tests/test_gpu_heap_codes_depth.py."""
import numpy as np
import pytest

from conftest import assert_bits_equal, oracle_both
from heap_pair_cases import _check_against_oracle, _device_sinks, _mixed_pairs
from suchtree_amd import _capi, synth
from suchtree_amd.exceptions import InvalidNodeError

pytestmark = pytest.mark.gpu

MIN_BATCH = 4096
TAILS = [1, 2, 3, 63, 1025]
DEFAULT_MIN_LEVELS = 19      # launch_policy.h: kHeapCodesDefaultMinLevels


def _codes_handle(parent, dist):
    dev = _capi.DeviceTree(parent, dist)
    dev.set_option("heap_lines", 2)
    dev.set_option("heap_codes", 2)
    return dev


@pytest.fixture(scope="module", params=[6, 7])
def codes_tree(request):
    """The handle, and three batches with the oracle's answers: every leaf pair, the same shifted by one position, a mix."""
    levels = request.param
    parent, dist = synth.balanced_tree(levels)
    dev = _codes_handle(parent, dist)
    info = dev.info()
    assert info["heap_codes"] == 1 and info["heap_lines"] == 1 and info["big_batch_kernel"] == "canopy", info
    assert (info["a_side_bytes"], info["b_table_bytes_per_leaf"]) == (4, 4), info
    ids = np.arange(0, len(parent), 2)
    a, b = np.meshgrid(ids, ids, indexing="ij")
    every = np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int64)
    assert len(every) == 4 ** levels
    batches = {"every leaf pair": every, "shifted by one": np.ascontiguousarray(np.roll(every, 1, axis=0)),
               "mixed": _mixed_pairs(len(parent), MIN_BATCH + max(TAILS), seed=levels)}
    want = {}
    for name, pairs in batches.items():
        d, m = oracle_both(parent, dist, pairs)
        d.setflags(write=False)
        m.setflags(write=False)
        want[name] = (d, m)
    yield levels, dev, batches, want
    dev.close()


def _set_hint(dev, hint):
    dev.set_option("stream_hint", hint)
    assert dev.info()["stream_hint"] == hint, dev.info()      # (0, or 1: the default covers what the heap-line form takes)


@pytest.mark.parametrize("batch", ["every leaf pair", "shifted by one"])
@pytest.mark.parametrize("hint", [0, 1])
def test_every_leaf_pair_on_either_lane_parity_every_sink(codes_tree, batch, hint):
    """k_canopy_ilp_codes<SrcContig>, both copies of its loop."""
    import torch
    levels, dev, batches, want = codes_tree
    try:
        _set_hint(dev, hint)
        pairs = batches[batch]
        got = _device_sinks(dev, torch.from_numpy(pairs).cuda(), len(pairs))
        _check_against_oracle(got, *want[batch], "%d levels, %s, stream_hint %d" % (levels, batch, hint))
    finally:
        dev.set_option("stream_hint", 1)


@pytest.mark.parametrize("batch", ["every leaf pair", "shifted by one", "mixed"])
def test_int32_pairs_through_the_host_path(codes_tree, batch):
    """k_canopy_ilp_codes<SrcContig32>, the 8-byte and the packed form of the source."""
    levels, dev, batches, want = codes_tree
    p32 = np.ascontiguousarray(batches[batch].astype(np.int32))
    try:
        for wire48 in (0, 1):
            dev.set_option("wire48", wire48)
            d, m = dev.distances_host(p32, True, True)
            what = "%d levels, %s, wire48 %d" % (levels, batch, wire48)
            assert_bits_equal(d, want[batch][0], what)
            assert np.array_equal(m, want[batch][1]), what
    finally:
        dev.set_option("wire48", 1)


@pytest.mark.parametrize("tail", TAILS)
def test_tails_with_internal_nodes_and_equal_ids(codes_tree, tail):
    import torch
    levels, dev, batches, want = codes_tree
    n = MIN_BATCH + tail
    pairs = batches["mixed"]
    t = torch.from_numpy(pairs).cuda()
    try:
        for hint in (0, 1):
            _set_hint(dev, hint)
            _check_against_oracle(_device_sinks(dev, t, n), want["mixed"][0][:n], want["mixed"][1][:n],
                                  "%d levels, %d pairs, stream_hint %d" % (levels, n, hint))
    finally:
        dev.set_option("stream_hint", 1)
    d, m = dev.distances_host(np.ascontiguousarray(pairs[:n].astype(np.int32)), True, True)
    assert_bits_equal(d, want["mixed"][0][:n], "%d levels, %d pairs, host path" % (levels, n))
    assert np.array_equal(m, want["mixed"][1][:n])


def test_out_of_range_ids_are_reported(codes_tree):
    """Fault record, NaN and -1, exactly as the other canopy kernels answer."""
    import torch
    levels, dev, batches, want = codes_tree
    n = MIN_BATCH + 3
    bad = batches["mixed"][:n].copy()
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
    assert_bits_equal(d[ok], want["mixed"][0][:n][ok])
    assert np.array_equal(m[ok], want["mixed"][1][:n][ok])


def test_codes_against_heap_lines_on_the_same_handle(codes_tree):
    import torch
    levels, dev, batches, want = codes_tree
    pairs = np.concatenate([batches["every leaf pair"], batches["mixed"]])
    n = len(pairs)
    t = torch.from_numpy(pairs).cuda()
    got = {}
    try:
        for codes in (0, 2):
            dev.set_option("heap_codes", codes)
            info = dev.info()
            assert info["heap_codes"] == (1 if codes else 0) and info["heap_lines"] == 1, info
            assert (info["a_side_bytes"], info["b_table_bytes_per_leaf"], info["stream_hint"]) == (4, 4, 1), info
            out_d = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            out_m = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
            dev.fault_check()
            got[codes] = (out_d, out_m)
    finally:
        dev.set_option("heap_codes", 2)
    assert torch.equal(got[0][0].view(torch.int64), got[2][0].view(torch.int64)) and torch.equal(got[0][1], got[2][1])
    # heap_lines 0 turns both forms off
    dev.set_option("heap_lines", 0)
    try:
        info = dev.info()
        assert info["heap_codes"] == 0 and info["heap_lines"] == 0, info
    finally:
        dev.set_option("heap_lines", 2)


@pytest.mark.parametrize("levels", [6, 7])
def test_a_tree_with_one_edge_without_a_code_keeps_the_heap_lines(levels):
    import torch
    parent, dist = synth.balanced_tree(levels)
    dist = dist.copy()
    dist[2 * 37] = np.float32(0.1234567)
    dev = _codes_handle(parent, dist)
    info = dev.info()
    assert info["heap_codes"] == 0 and info["heap_lines"] == 1 and (info["a_side_bytes"], info["b_table_bytes_per_leaf"]) == (4, 4), info
    pairs = _mixed_pairs(len(parent), MIN_BATCH + 63, seed=levels)
    pairs[::5, 0] = 2 * 37      # (the edge itself, often)
    want_d, want_m = oracle_both(parent, dist, pairs)
    n = len(pairs)
    t = torch.from_numpy(pairs).cuda()
    out_d = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    out_m = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
    dev.fault_check()
    assert_bits_equal(out_d.cpu().numpy(), want_d, "refused tree")
    assert np.array_equal(out_m.cpu().numpy(), want_m)
    dev.close()


def test_option_values_and_the_default_handle_of_2_17_leaves():
    dev = _capi.DeviceTree(*synth.balanced_tree(17))
    for value in (-1, 3):
        with pytest.raises(ValueError):
            dev.set_option("heap_codes", value)
    info = dev.info()
    assert info["heap_codes"] == (1 if 17 >= DEFAULT_MIN_LEVELS else 0), info
    assert info["heap_lines"] == 1 and (info["a_side_bytes"], info["b_table_bytes_per_leaf"]) == (4, 4), info
    dev.set_option("heap_codes", 2)
    assert dev.info()["heap_codes"] == 1
    dev.set_option("heap_codes", 0)
    assert dev.info()["heap_codes"] == 0 and dev.info()["heap_lines"] == 1
    dev.close()
