"""Call-scoped device scratch comes back: the host calls that allocate a block, a stream or a handful of buffers for
one call (st_compare_*_host, st_quartet_positions, st_knn_host; device_res.h owns them) return it on success and on
their error exits, and a handle serves the same bits after an error as before it.

Every call below holds at least 8 MiB of device memory while it runs, so twenty leaked calls would pass the 64 MiB bar
of test_gpu_host_path.py::test_create_destroy_cycles_do_not_leak_device_or_pinned_memory, which is this test's bar too.
"""
import numpy as np
import pytest

from suchtree_amd import _capi, synth
from suchtree_amd.exceptions import InvalidNodeError

pytestmark = pytest.mark.gpu

ROWS_CHUNK_BLOCKS = 1 << 18          # compare_plan.h: kRowsChunkBlocks
BAR = 64 << 20


def test_scratch_of_host_calls_comes_back_on_success_and_on_error_exits():
    import torch
    parent, dist = synth.balanced_tree(12)
    n_nodes = len(parent)
    d = _capi.DeviceTree(parent, dist)
    other = d                        # the same tree as "other": one pipe mutex, taken once
    rng = np.random.default_rng(2026)
    leaves = np.arange(1 << 12, dtype=np.int64) * 2

    pairs_x, pairs_y = rng.choice(leaves, (1 << 20, 2)), rng.choice(leaves, (1 << 20, 2))      # a 24 MiB block
    n_rows = 2 * ROWS_CHUNK_BLOCKS + 1001      # (test_gpu_reductions.py: many tiny rows over three chunks)
    rows_x, rows_y = rng.choice(leaves, (n_rows, 3)), rng.choice(leaves, (n_rows, 3))
    link_x, link_y = rng.choice(leaves, 900), rng.choice(leaves, 900)      # (test_gpu_reductions.py: 900 links)
    # four distinct leaves a row (the host's draw), another order in the other tree: a 28 MiB block
    quartets_x = leaves[_capi.quartet_positions("sample", 7, len(leaves), 0, 1 << 18)]
    quartets_y = np.ascontiguousarray(quartets_x[:, [2, 0, 3, 1]])
    small_quartets = quartets_x[:1 << 16]
    queries, cands = rng.integers(0, n_nodes, 1024), rng.integers(0, n_nodes, 8192)      # a 32 MiB distance block

    def moments_and(second):
        return lambda r: bytes(r[0]) + bytes(second(r[1]))

    good = {
        "compare_pairs": (lambda: d.compare_pairs_host(other, pairs_x, pairs_y), lambda r: bytes(r[0])),
        "compare_pairs_ranks": (lambda: d.compare_pairs_ranks_host(other, pairs_x, pairs_y), moments_and(bytes)),
        "compare_rows": (lambda: d.compare_rows_host(other, rows_x, rows_y), lambda r: r.tobytes()),
        "compare_clades": (lambda: d.compare_clades_host(other, parent, link_x, link_y), lambda r: r[0].tobytes() + r[1].tobytes()),
        "compare_quartets": (lambda: d.compare_quartets_host(other, quartets_x, quartets_y), lambda r: r.tobytes()),
        "compare_quartets_leaves": (lambda: d.compare_quartets_leaves_host(other, leaves, leaves[::-1].copy(), mode="sample", seed=9,
                                                                           k_count=1 << 18), lambda r: r.tobytes()),
        "quartet_positions": (lambda: _capi.quartet_positions("sample", 9, len(leaves), 0, 1 << 20, device=0), lambda r: r.tobytes()),
        "knn": (lambda: d.knn_host(queries, cands, 3), lambda r: r[0].tobytes() + r[1].tobytes()),
        "quartets": (lambda: d.quartets_host(small_quartets), lambda r: r.tobytes()),
    }

    def bits(name):
        call, as_bytes = good[name]
        return as_bytes(call())

    # error exits, each followed by the good call of the same entry point
    bad_cands = cands.copy()
    bad_cands[4321] = n_nodes                  # found by the kernels: the call unwinds with work behind it
    bad_quartets = small_quartets.copy()
    bad_quartets[777, 2] = -5
    bad_pairs = pairs_x.copy()
    bad_pairs[5, 1] = n_nodes + 7              # found by the host check, before anything is allocated
    errors = {
        "knn": (lambda: d.knn_host(queries, bad_cands, 3), n_nodes),
        "quartets": (lambda: d.quartets_host(bad_quartets), -5),
        "compare_pairs": (lambda: d.compare_pairs_host(other, bad_pairs, pairs_y), n_nodes + 7),
    }

    first = {}

    def one_round(with_errors):
        for name in good:
            if with_errors and name in errors:
                call, bad_id = errors[name]
                with pytest.raises(InvalidNodeError) as err:
                    call()
                assert err.value.node_id == bad_id, name
            got = bits(name)
            assert got == first.setdefault(name, got), name + (" after an error exit" if with_errors and name in errors else "")

    for _ in range(3):                         # warm-up: what a handle keeps between calls (pipe, q_tmp, mailbox) exists
        one_round(True)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for it in range(20):
        one_round(it % 3 == 2)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print("free device memory: %d MiB before, %d MiB after 20 rounds" % (free0 >> 20, free1 >> 20))
    assert abs(free0 - free1) < BAR, "free device memory moved by %d MiB over 20 rounds of host calls" % ((free0 - free1) >> 20)
    d.close()
