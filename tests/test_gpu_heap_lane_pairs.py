"""The lane pairs of k_canopy_ilp_heap on the GPU against the oracle, by bits: lanes l and l ^ 1 share their line loads (either
gather instruction reads the window of one lane's slot and, on the lane beside it, the top of the same slot; quad permutes hand
the values over), so what a lane computes now depends on where it sits and on what its neighbour holds.  Perfect trees of 6
and 7 levels (64 and 128 leaves, 4 and 8 lines: the smallest the form serves) with option heap_lines = 2; every batch goes
through every cell: the float64, float32, int32-id and 24-bit-id sinks of the device path with stream_hint 0 and 1 (both copies
of the loop), and int32 pairs through the host path.  Batches have at least 4096 pairs (smaller ones never reach the kernel)."""
import numpy as np
import pytest

from conftest import assert_bits_equal, oracle_both
from suchtree_amd import sharding
from suchtree_amd.exceptions import InvalidNodeError
from test_gpu_heap_lines import MIN_BATCH, _all_pairs, _heap_tree, _tile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[6, 7])
def tree(request):
    parent, dist, dev = _heap_tree(request.param)
    yield request.param, parent, dist, dev
    dev.close()


def _oracle(parent, dist, pairs):
    """(distances, ids, in range) with NaN and -1 where an id is out of range"""
    ok = ((pairs >= 0) & (pairs < len(parent))).all(axis=1)
    want_d, want_m = oracle_both(parent, dist, np.where(ok[:, None], pairs, 0))
    want_d[~ok], want_m[~ok] = np.nan, -1
    return want_d, want_m, ok


def _same(got_d, got_m, want_d, want_m, ok, what):
    got_d = np.asarray(got_d, np.float64)
    assert np.isnan(got_d[~ok]).all() and (got_m[~ok] == -1).all(), what
    assert_bits_equal(got_d[ok], want_d[ok], what)
    assert np.array_equal(got_m[ok], want_m[ok]), what


def _every_cell(dev, parent, dist, pairs, what):
    import torch
    pairs = np.ascontiguousarray(pairs, np.int64)
    n = len(pairs)
    assert n >= MIN_BATCH
    want_d, want_m, ok = _oracle(parent, dist, pairs)
    t = torch.from_numpy(pairs).cuda()
    pb = sharding.packed_bytes(n)
    try:
        for hint in (0, 1):
            dev.set_option("stream_hint", hint)
            assert dev.info()["stream_hint"] == hint and dev.info()["heap_lines"] == 1, dev.info()
            d64 = torch.full((n + 4,), -7.0, dtype=torch.float64, device="cuda")
            m_a = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
            dev.distances_device(t.data_ptr(), n, d64.data_ptr(), m_a.data_ptr())
            f32 = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
            m_b = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
            dev.distances_device(t.data_ptr(), n, f32.data_ptr(), m_b.data_ptr(), f32=True)
            w32 = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
            m24 = torch.full((pb + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            dev.distances_device_wire(t.data_ptr(), n, w32.data_ptr(), m24.data_ptr())
            m_c = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
            dev.unpack_mrca24_device(m24.data_ptr(), n, m_c.data_ptr())
            if ok.all():
                dev.fault_check()
            else:
                with pytest.raises(InvalidNodeError) as e:
                    dev.fault_check()
                assert e.value.node_id in set(pairs[~ok].ravel().tolist()) - set(range(len(parent))), what
            for buf, canary in ((d64, -7.0), (f32, -7.0), (w32, -7.0), (m_a, -9), (m_b, -9), (m_c, -9)):
                assert bool((buf[n:] == canary).all()), what + ": a store past the last pair"
            assert bool((m24[pb:] == 0xEE).all()), what + ": a store past the packed ids"
            for sink, d, m in (("float64", d64, m_a), ("float32", f32, m_b), ("wire", w32, m_c)):
                _same(d[:n].cpu().numpy(), m[:n].cpu().numpy(), want_d, want_m, ok, "%s, stream_hint %d, %s sink" % (what, hint, sink))
    finally:
        dev.set_option("stream_hint", 1)
    p32 = np.ascontiguousarray(pairs.astype(np.int32))
    assert np.array_equal(p32, pairs)      # (every id of these batches fits: the int32 source sees the same pairs)
    if ok.all():
        d, m = dev.distances_host(p32, True, True)
        _same(d, m, want_d, want_m, ok, what + ": int32 pairs through the host path")
    else:
        with pytest.raises(InvalidNodeError):
            dev.distances_host(p32, True, True)


def test_every_leaf_pair_on_an_even_and_on_an_odd_lane():
    """All 4096 leaf pairs of the 64-leaf tree as batch P and as P[1:]: every pair is computed once on an even and once on an
    odd lane, beside both of its neighbours in P."""
    parent, dist, dev = _heap_tree(6)
    twice = _tile(_all_pairs(np.arange(0, len(parent), 2)), 2 * MIN_BATCH)
    assert len(twice) == 2 * MIN_BATCH
    _every_cell(dev, parent, dist, twice, "P")
    _every_cell(dev, parent, dist, twice[1:], "P[1:]")
    dev.close()


def _leaf_pairs(levels, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << levels, (n, 2)).astype(np.int64) * 2


def _other(kind, levels, n_nodes, beside, seed):
    """The pairs that sit beside the leaf pairs `beside`, lane for lane."""
    rng = np.random.default_rng(seed)
    n = len(beside)
    if kind == "internal":      # an internal node on either side or on both
        other = rng.integers(0, n_nodes - 1, (n, 2))      # (the last id is a leaf's: | 1 stays inside the tree)
        other[np.arange(n), rng.integers(0, 2, n)] |= 1
    elif kind == "out of range":
        other = _leaf_pairs(levels, n, seed + 1)
        other[np.arange(n), rng.integers(0, 2, n)] = rng.choice([-3, -1, n_nodes, n_nodes + 5, 2**31 - 1], n)
    elif kind == "a == b":
        other = np.repeat(rng.integers(0, 1 << levels, n)[:, None], 2, axis=1) * 2
    else:                       # "neighbour's line": either node from the line of 16 leaves that the neighbour's node is read from
        assert kind == "neighbour's line"
        other = (((beside >> 1) & ~15) | rng.integers(0, 16, (n, 2))) * 2
    return other.astype(np.int64)


@pytest.mark.parametrize("leaf_pairs_on", ["even", "odd"])
@pytest.mark.parametrize("kind", ["internal", "out of range", "a == b", "neighbour's line"])
def test_unequal_neighbours(tree, kind, leaf_pairs_on):
    """Leaf pairs on the lanes of one parity, and beside each of them a pair that takes another way through the kernel (slot 0
    and the walk; slot 0, NaN / -1 and the fault; no climb at all) or reads the very same lines."""
    levels, parent, dist, dev = tree
    n = MIN_BATCH + 512
    leaf = _leaf_pairs(levels, n // 2, seed=levels)
    other = _other(kind, levels, len(parent), leaf, seed=10 * levels + len(kind))
    pairs = np.empty((n, 2), np.int64)
    first = 0 if leaf_pairs_on == "even" else 1
    pairs[first::2], pairs[1 - first::2] = leaf, other
    _every_cell(dev, parent, dist, pairs, "%d levels, %s beside leaf pairs on %s lanes" % (levels, kind, leaf_pairs_on))


@pytest.mark.parametrize("extra", [1, 2, 3, 63, 1025])
def test_tails(tree, extra):
    """The last live lane's neighbour has no pair (+ 1, + 3, + 63, + 1025), or the last two lanes hold the last two pairs (+ 2)."""
    levels, parent, dist, dev = tree
    n = MIN_BATCH + extra
    pairs = _leaf_pairs(levels, n, seed=100 + levels)
    pairs[-1] = (2 * ((1 << levels) - 1), 0)      # (the last pair: the tree's last line on a's side)
    _every_cell(dev, parent, dist, pairs, "%d levels, %d pairs" % (levels, n))
