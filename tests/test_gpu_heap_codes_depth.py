"""The heap-code form of the predicated kernel (k_canopy_ilp_codes) at depth and over more than one trip of its grid, on the
GPU against the oracle, by bits.  tests/test_gpu_heap_codes.py stops at 7 levels (one edge above the line at the most) and at
16,384 pairs (one trip of the loop over the pairs); here the trees have 8 levels (the first depth with two edges in the heap
image), 13, 19 (the largest image that needs no grant of LDS, 64 KiB, and the lower edge of the default policy) and 20 (128 KiB,
granted per kernel; the headline tree and the maximum), and the batches are
  every k          as many pairs for every number of edges k = 0 .. levels between a leaf and the MRCA, with k the same over a
                   wave and shuffled (heap_pair_cases.by_k_pairs): every term of the climb is the last one added equally often;
  edge slots       the slots at which the code lines begin and end, the last line, which is not full, among them;
  trips            3 * 1024 * CUs + 1025 pairs, the shuffled every-k batch and then the mixed batch with internal nodes and equal
                   ids: launch_heap_family starts at most CUs workgroups of 1024 lanes, so the loop of heap_pairs takes four
                   trips; prefixes of 2 * 1024 * CUs pairs and of 1 and 63 more end beside a full grid;
through every sink between canaries with both values of the streaming hint, as int32 through the host path in both wire forms,
against the heap lines on the same handle, with one id out of range in the first trip and one in the third, and -- on the
19-level tree -- 2^24 and 2^24 - 1 pairs on a default handle, which the policy sends to the codes and to the heap lines."""
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal
from heap_pair_cases import _check_against_oracle, _device_sinks, _mixed_pairs, by_k_pairs, edge_slot_pairs, oracle_answers
from oracle.oracle import OracleTree
from suchtree_amd import _capi, synth
from suchtree_amd.exceptions import InvalidNodeError

pytestmark = pytest.mark.gpu

LEVELS = (8, 13, 19, 20)
BLOCK = 1024                     # launch_geometry.h: kCanopyBlock
DEFAULT_MIN_LEVELS = 19          # launch_policy.h: kHeapCodesDefaultMinLevels
DEFAULT_MIN_PAIRS = 1 << 24      # launch_policy.h: kHeapCodesDefaultMinPairs


@functools.lru_cache(maxsize=None)
def _tree(levels):
    parent, dist = synth.balanced_tree(levels)
    return parent, dist, OracleTree(parent, dist)


def _grid():
    """Lanes of the largest grid launch_heap_family starts: one workgroup of 1024 lanes per CU."""
    import torch
    return BLOCK * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", params=LEVELS)
def deep(request):
    """Per level: the handle with the form forced, and the batches with the oracle's answers (one OracleTree, one call)."""
    levels = request.param
    parent, dist, oracle = _tree(levels)
    dev = _capi.DeviceTree(parent, dist)
    dev.set_option("heap_lines", 2)
    dev.set_option("heap_codes", 2)
    info = dev.info()
    assert info["heap_codes"] == 1 and info["heap_lines"] == 1 and info["big_batch_kernel"] == "canopy", info
    grouped, shuffled = by_k_pairs(levels, 4096, seed=300 + levels)
    n_trips = 3 * _grid() + BLOCK + 1
    batches = {"every k, grouped": grouped, "every k, shuffled": shuffled, "edge slots": edge_slot_pairs(levels, seed=400 + levels),
               "trips": np.concatenate([shuffled, _mixed_pairs(len(parent), n_trips - len(shuffled), seed=500 + levels)])}
    assert len(batches["trips"]) == n_trips
    every = np.concatenate(list(batches.values()))
    d, m = oracle_answers(oracle, every)
    want, lo = {}, 0
    for name, pairs in batches.items():
        want[name] = (d[lo:lo + len(pairs)], m[lo:lo + len(pairs)])
        lo += len(pairs)
    yield levels, dev, batches, want
    dev.close()


def _set_hint(dev, hint):
    dev.set_option("stream_hint", hint)
    assert dev.info()["stream_hint"] == hint, dev.info()


def _every_call(dev, pairs, want, what, prefixes=None):
    """The first n pairs for every n of `prefixes` (default: all) through every device sink under both hints, and all of them
    as int32 through the host path in both forms of the source."""
    import torch
    want_d, want_m = want
    t = torch.from_numpy(np.ascontiguousarray(pairs)).cuda()
    try:
        for hint in (0, 1):
            _set_hint(dev, hint)
            for n in prefixes or (len(pairs),):
                _check_against_oracle(_device_sinks(dev, t, n), want_d[:n], want_m[:n], "%s, %d pairs, stream_hint %d" % (what, n, hint))
    finally:
        dev.set_option("stream_hint", 1)
    p32 = np.ascontiguousarray(pairs.astype(np.int32))
    try:
        for wire48 in (0, 1):
            dev.set_option("wire48", wire48)
            d, m = dev.distances_host(p32, True, True)
            assert_bits_equal(d, want_d, "%s, host path, wire48 %d" % (what, wire48))
            assert np.array_equal(m, want_m), (what, wire48)
    finally:
        dev.set_option("wire48", 1)


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_every_k(deep, order):
    """Every predicate kHeapLineEdges + q < k of either side's climb false for the first time equally often."""
    levels, dev, batches, want = deep
    name = "every k, " + order
    _every_call(dev, batches[name], want[name], "%d levels, %s" % (levels, name))


def test_edge_slots(deep):
    levels, dev, batches, want = deep
    _every_call(dev, batches["edge slots"], want["edge slots"], "%d levels, edge slots" % levels)


def test_more_pairs_than_one_trip_of_the_grid(deep):
    """Four trips of heap_pairs' loop over `base` under CodeSide, the last one with 1025 pairs; two trips exactly, and 1 and 63
    pairs more (the third trip's only workgroup beside CUs - 1 that are done)."""
    levels, dev, batches, want = deep
    grid, n = _grid(), len(batches["trips"])
    assert n == 3 * grid + 1025
    _every_call(dev, batches["trips"], want["trips"], "%d levels, trips" % levels, prefixes=(n, 2 * grid, 2 * grid + 1, 2 * grid + 63))


def test_codes_against_heap_lines_on_the_same_handle(deep):
    import torch
    levels, dev, batches, want = deep
    pairs = batches["trips"]
    n = len(pairs)
    t = torch.from_numpy(pairs).cuda()
    got = {}
    try:
        for codes in (0, 2):
            dev.set_option("heap_codes", codes)
            info = dev.info()
            assert info["heap_codes"] == (1 if codes else 0) and info["heap_lines"] == 1, info
            out_d = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            out_m = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
            dev.fault_check()
            got[codes] = (out_d, out_m)
    finally:
        dev.set_option("heap_codes", 2)
    assert torch.equal(got[0][0].view(torch.int64), got[2][0].view(torch.int64)) and torch.equal(got[0][1], got[2][1])
    assert_bits_equal(got[2][0].cpu().numpy(), want["trips"][0], "%d levels, codes" % levels)


def test_out_of_range_ids_in_the_first_and_the_third_trip(deep):
    """Fault record, NaN and -1 for the two pairs, every other cell as the oracle has it."""
    import torch
    levels, dev, batches, want = deep
    n = len(batches["trips"])
    bad_at = [5, 2 * _grid() + 4097]
    bad = batches["trips"].copy()
    bad[bad_at[0], 0], bad[bad_at[1], 1] = -3, 1 << 40
    t = torch.from_numpy(bad).cuda()
    out_d = torch.zeros(n, dtype=torch.float64, device="cuda")
    out_m = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
    with pytest.raises(InvalidNodeError):
        dev.fault_check()
    d, m = out_d.cpu().numpy(), out_m.cpu().numpy()
    ok = np.ones(n, bool)
    ok[bad_at] = False
    assert np.isnan(d[~ok]).all() and (m[~ok] == -1).all()
    assert_bits_equal(d[ok], want["trips"][0][ok])
    assert np.array_equal(m[ok], want["trips"][1][ok])


def test_default_policy_at_its_lower_edges():
    """A handle with no option set on the 19-level tree: 2^24 pairs go to the codes and 2^24 - 1 to the heap lines.  Either
    batch gives the same bytes under heap_codes 0, 1 and 2, and a sample of 100,000 positions is the oracle's."""
    import torch
    levels = DEFAULT_MIN_LEVELS
    parent, dist, oracle = _tree(levels)
    dev = _capi.DeviceTree(parent, dist)
    info = dev.info()
    assert info["heap_codes"] == 1 and info["heap_lines"] == 1 and info["big_batch_kernel"] == "canopy", info
    gen = torch.Generator(device="cuda")
    gen.manual_seed(levels)
    t = torch.randint(0, 1 << levels, (DEFAULT_MIN_PAIRS, 2), generator=gen, device="cuda", dtype=torch.int64) * 2
    rng = np.random.default_rng(levels)
    try:
        for n in (DEFAULT_MIN_PAIRS, DEFAULT_MIN_PAIRS - 1):
            at = np.unique(np.concatenate([rng.integers(0, n, 100_000 - 3), [0, n - 2, n - 1]]))
            at_t = torch.from_numpy(at).cuda()
            want_d, want_m = oracle_answers(oracle, t[at_t].cpu().numpy())
            first = None
            for codes in (1, 0, 2):
                dev.set_option("heap_codes", codes)
                out_d = torch.full((DEFAULT_MIN_PAIRS,), -7.0, dtype=torch.float64, device="cuda")
                out_m = torch.full((DEFAULT_MIN_PAIRS,), -9, dtype=torch.int32, device="cuda")
                dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
                dev.fault_check()
                what = "%d pairs, heap_codes %d" % (n, codes)
                assert bool((out_d[n:] == -7.0).all()) and bool((out_m[n:] == -9).all()), what
                if first is None:
                    first = (out_d, out_m)
                    assert_bits_equal(out_d[at_t].cpu().numpy(), want_d, what)
                    assert np.array_equal(out_m[at_t].cpu().numpy(), want_m), what
                else:
                    assert torch.equal(first[0].view(torch.int64), out_d.view(torch.int64)) and torch.equal(first[1], out_m), what
                del out_d, out_m
    finally:
        dev.close()
