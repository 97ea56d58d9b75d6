"""The streaming hint (option "stream_hint"; device_common.h) on the GPU: the non-temporal loads of the pair source and stores of
the result sinks give the oracle's bits, the same bits as the plain form, and touch nothing outside their ranges -- on both
instantiations of the heap-line kernel (int64 pairs in device buffers: both copies of its loop; int32 pairs through the host
path: the plain loop under either option value), at batch sizes with tail waves, a tail quad of the packed sink and a partial
last workgroup, with offset pointers, with an id out of range, and on the kernels of general tables (k_canopy_ilp takes the
hinted pair load with option value 2).  Batches have at least 4096 pairs (smaller ones never reach the canopy
kernels)."""
import numpy as np
import pytest

from conftest import assert_bits_equal, oracle_both
from suchtree_amd import _capi, sharding, synth
from suchtree_amd.exceptions import InvalidNodeError

pytestmark = pytest.mark.gpu

SIZES = [4096, 4097, 4099, 5183]
N_MAX = max(SIZES) + 1      # (+ 1: the launch whose pair pointer is advanced by one pair)
DEFAULT_HINT_2_18 = 1       # what launch_policy.h decides for a default handle of 2^18 leaves (the heap-line kernel takes its batches)


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


def _set_hint(dev, hint):
    dev.set_option("stream_hint", hint)
    assert dev.info()["stream_hint"] == (1 if hint == 2 else 0), dev.info()


@pytest.fixture(scope="module", params=[6, 7, 10])
def heap_tree(request):
    levels = request.param
    parent, dist = synth.balanced_tree(levels)
    dev = _capi.DeviceTree(parent, dist)
    dev.set_option("heap_lines", 2)
    assert dev.info()["heap_lines"] == 1, dev.info()
    pairs = _mixed_pairs(len(parent), N_MAX, seed=levels)
    want_d, want_m = oracle_both(parent, dist, pairs)
    want_d.setflags(write=False)
    want_m.setflags(write=False)
    yield levels, dev, pairs, want_d, want_m
    dev.close()


def _device_sinks(dev, t_pairs, first, n):
    """Every sink of the device entry points for pairs [first, first + n): float64 + int32, float32 + int32, and the wire form
    (float32 + packed ids, unpacked on the same stream right after the launch).  Outputs start at element 4 of larger buffers
    between canaries (-7.0, -9, 0xEE bytes), which must survive."""
    import torch
    ptr = t_pairs.data_ptr() + 16 * first
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
    if 3 * n < pb:      # (padding bytes of the last dword: the kernel writes zeros there or nothing)
        assert all(int(x) in (0, 0xEE) for x in m24[16 + 3 * n:16 + pb].cpu()), "padding of the packed ids"
    return [x[4:n + 4].cpu().numpy() for x in (d64, m_a, f32, m_b, w32, m_c)]


def _check_against_oracle(got, want_d, want_m, what):
    d64, m_a, f32, m_b, w32, m_c = got
    assert_bits_equal(d64, want_d, what + ": float64 sink")
    assert_bits_equal(f32.astype(np.float64), want_d, what + ": float32 sink")
    assert_bits_equal(w32.astype(np.float64), want_d, what + ": wire sink")
    for m in (m_a, m_b, m_c):
        assert np.array_equal(m, want_m), what


@pytest.mark.parametrize("n", SIZES)
def test_heap_kernel_device_sinks(heap_tree, n):
    """k_canopy_ilp_heap<SrcContig>: stream_hint 0 and 2 against the oracle and against each other, by bits."""
    import torch
    levels, dev, pairs, want_d, want_m = heap_tree
    t = torch.from_numpy(pairs).cuda()
    got = {}
    for hint in (0, 2):
        _set_hint(dev, hint)
        got[hint] = _device_sinks(dev, t, 0, n)
        _check_against_oracle(got[hint], want_d[:n], want_m[:n], "%d levels, %d pairs, stream_hint %d" % (levels, n, hint))
    for plain, hinted in zip(got[0], got[2]):
        assert plain.tobytes() == hinted.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_heap_kernel_int32_pairs_through_the_host_path(heap_tree, n):
    """k_canopy_ilp_heap<SrcContig32>, the 8-byte and the packed form of the source (this instantiation keeps the plain loop: the
    option must change nothing)."""
    levels, dev, pairs, want_d, want_m = heap_tree
    p32 = np.ascontiguousarray(pairs[:n].astype(np.int32))
    try:
        for wire48 in (0, 1):
            dev.set_option("wire48", wire48)
            for hint in (0, 2):
                _set_hint(dev, hint)
                d, m = dev.distances_host(p32, True, True)
                what = "%d levels, %d pairs, wire48 %d, stream_hint %d" % (levels, n, wire48, hint)
                assert_bits_equal(d, want_d[:n], what)
                assert np.array_equal(m, want_m[:n]), what
    finally:
        dev.set_option("wire48", 1)


def test_pair_pointer_advanced_by_one_pair(heap_tree):
    """The pair array is 16-byte aligned and no more: a launch that starts at its second pair."""
    import torch
    levels, dev, pairs, want_d, want_m = heap_tree
    t = torch.from_numpy(pairs).cuda()
    n = N_MAX - 1
    for hint in (0, 2):
        _set_hint(dev, hint)
        _check_against_oracle(_device_sinks(dev, t, 1, n), want_d[1:], want_m[1:], "%d levels, from pair 1, stream_hint %d" % (levels, hint))


def test_id_out_of_range_with_the_hint(heap_tree):
    import torch
    levels, dev, pairs, want_d, want_m = heap_tree
    n = 4099
    bad = pairs[:n].copy()
    bad_id = len(want_m) * 1000 + 12345
    bad[4097, 1] = bad_id
    _set_hint(dev, 2)
    t = torch.from_numpy(bad).cuda()
    out_d = torch.zeros(n, dtype=torch.float64, device="cuda")
    out_m = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev.distances_device(t.data_ptr(), n, out_d.data_ptr(), out_m.data_ptr())
    with pytest.raises(InvalidNodeError) as e:
        dev.fault_check()
    assert str(bad_id) in str(e.value) and e.value.node_id == bad_id
    d, m = out_d.cpu().numpy(), out_m.cpu().numpy()
    ok = np.ones(n, bool)
    ok[4097] = False
    assert np.isnan(d[4097]) and m[4097] == -1
    assert_bits_equal(d[ok], want_d[:n][ok])
    assert np.array_equal(m[ok], want_m[:n][ok])


@pytest.mark.parametrize("tree", ["perfect 2^12 without heap lines", "random 4000 leaves"])
def test_general_tables(tree):
    """k_canopy_ilp (hinted pair loads with option value 2) and whatever else the handle chooses."""
    import torch
    if tree.startswith("perfect"):
        parent, dist = synth.balanced_tree(12)
    else:
        parent, dist = synth.random_binary_tree(4000, seed=8)[:2]
    dev = _capi.DeviceTree(parent, dist)
    dev.set_option("heap_lines", 0)
    assert dev.info()["heap_lines"] == 0
    pairs = _mixed_pairs(len(parent), 5183, seed=12)
    want_d, want_m = oracle_both(parent, dist, pairs)
    t = torch.from_numpy(pairs).cuda()
    got = {}
    for hint in (0, 2):
        _set_hint(dev, hint)
        got[hint] = _device_sinks(dev, t, 0, len(pairs))
        _check_against_oracle(got[hint], want_d, want_m, "%s, stream_hint %d" % (tree, hint))
    for plain, hinted in zip(got[0], got[2]):
        assert plain.tobytes() == hinted.tobytes()
    dev.close()


def test_option_and_info():
    dev = _capi.DeviceTree(*synth.balanced_tree(10))
    for value in (-1, 3):
        with pytest.raises(ValueError):
            dev.set_option("stream_hint", value)
    # default policy: where the heap-line kernel takes the batches (a 2^10-leaf tree: only when told to)
    assert dev.info()["heap_lines"] == 0 and dev.info()["stream_hint"] == 0
    dev.set_option("heap_lines", 2)
    assert dev.info()["heap_lines"] == 1 and dev.info()["stream_hint"] == 1
    dev.set_option("stream_hint", 0)
    assert dev.info()["stream_hint"] == 0
    dev.set_option("heap_lines", 0)
    dev.set_option("stream_hint", 2)
    assert dev.info()["heap_lines"] == 0 and dev.info()["stream_hint"] == 1
    dev.close()
    big = _capi.DeviceTree(*synth.balanced_tree(18))
    info = big.info()
    assert info["stream_hint"] == DEFAULT_HINT_2_18 and info["stream_hint"] == info["heap_lines"], info
    big.close()
