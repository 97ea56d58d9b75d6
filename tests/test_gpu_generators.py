"""The result-returning pair generators (SrcTriangle, SrcGrid, SrcQuartet: triangle_host / triangle_device, grid_host,
quartets_host, knn_host) under every kernel form and at their edges, and the small kernels beside them (k_knn_select,
k_graph_*, k_unpack24).

Reference: the CPU oracle on the pairs a generator is DEFINED to produce, expanded on the host with plain integer code
(math.isqrt, np.divmod) -- never with sharding.triangle_row_of, which restates the device formula.  A call of up to
FULL_ORACLE_MAX pairs is checked against the oracle pair by pair; a larger one sends a seeded sample of at least
ORACLE_SAMPLE pairs plus the first and last LAUNCH_EDGE pairs of every launch to the oracle and compares the rest with the
same handle's explicit-pair result under strategy "walk" (pinned to the oracle by test_gpu_parity.py).  Everything is
compared bit for bit: distances as float64 bit patterns, ids equal.

Group A proves that it reached its kernel form from the library's own reported state (info(), st_host_chunk_plan) and
the thresholds restated below; a launch whose size leaves the kernel undetermined fails the test."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import assert_bits_equal, oracle_both
from oracle.oracle import OracleTree
from suchtree_amd import InvalidNodeError, SuchTree, _capi, synth

pytestmark = pytest.mark.gpu

CANOPY_MIN_PAIRS = 4096                  # launch_policy.h:76 kCanopyMinPairs: the smallest value canopy_min_pairs() returns
CANOPY_MIN_PAIRS_MAX = 524288            # launch_policy.h:131: the largest (with ladder_min_pairs <= it)
LADDER_MIN_PAIRS = 131072                # launch_policy.h:90 kLadderMinPairs
WALK_SORTED_MIN_PAIRS = 262144           # launch_policy.h:148 kWalkSortedMinPairs
PREFERS_WALK_SORTED_MIN = 524288         # launch_policy.h:154 prefers_walk_sorted
LADDER_DYNAMIC_MIN = 1 << 22             # launch_canopy.hip:48 kLadderDynamicMin (records of 512 bytes; 1 KB: half of it)
HOST_CHUNK_MIN, HOST_CHUNK_MAX = 1 << 18, 1 << 22      # host_path.h:16-17 kHostChunkMin / kHostChunk
QUARTET_CHUNK = HOST_CHUNK_MAX // 8      # host_quartets.h: quartets_host_run
KNN_BLOCK_ELEMS = 1 << 26                # host_misc.h: knn_host_run, rows_per_block
KNN_MAX_K = 256                          # kernels_misc.h:15 kKnnMaxK
GRAPH_SCATTER_SPAN = 4096 * 256          # host_misc.h: graph_matrices_run: edges one pass of k_graph_scatter covers
GRAPH_LAPLACIAN_SPAN = 65536 * 256       # host_misc.h: graph_matrices_run: elements one pass of k_graph_laplacian covers
TRIANGLE_MAX_M = 3_000_000_000           # host_compare.h: triangle_range_args

FULL_ORACLE_MAX = 1 << 20
ORACLE_SAMPLE = 200_000
LAUNCH_EDGE = 4096

THREADS = min(16, len(os.sched_getaffinity(0)))


def _leaves(parent):
    return np.flatnonzero(np.bincount(parent[parent >= 0], minlength=len(parent)) == 0).astype(np.int64)


def _T(r):
    """First pair index of triangle row r (row r holds the pairs (ids[c], ids[r]), c < r)."""
    return r * (r - 1) // 2


def _tri_rc(k0, count):
    """(row, col) of the triangle pairs k0 .. k0 + count - 1, k = row (row - 1) / 2 + col with 0 <= col < row: the row of k0
    from math.isqrt on Python integers, the rest by counting."""
    row = (1 + math.isqrt(1 + 8 * k0)) // 2
    col = k0 - _T(row)
    assert 0 <= col < row and _T(row) <= k0 < _T(row + 1)
    rows, cols = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    left = count
    while left > 0:
        take = min(left, row - col)
        rows.append(np.full(take, row, np.int64))
        cols.append(np.arange(col, col + take, dtype=np.int64))
        left -= take
        row, col = row + 1, 0
    return np.concatenate(rows), np.concatenate(cols)


def _tri_pairs(ids, k0, count):
    r, c = _tri_rc(k0, count)
    return np.stack([ids[c], ids[r]], 1)


def _grid_pairs(rows, cols, e0, count, symmetric=False):
    r, c = np.divmod(np.arange(e0, e0 + count, dtype=np.int64), len(cols))
    a, b = rows[r], cols[c]
    if symmetric:
        below = c < r
        a, b = np.where(below, b, a), np.where(below, a, b)
    return np.stack([a, b], 1)


def _oracle_quartets(parent, dist, q):
    """OracleTree.quartets over contiguous pieces on all host cores (one OracleTree per thread, as conftest.oracle_both)."""
    q = np.ascontiguousarray(q, dtype=np.int64)
    k = max(1, min(THREADS, len(q) // 256))
    bounds = [len(q) * i // k for i in range(k + 1)]
    with ThreadPoolExecutor(k) as ex:
        parts = list(ex.map(lambda i: OracleTree(parent, dist).quartets(q[bounds[i]:bounds[i + 1]]), range(k)))
    return np.concatenate(parts)


def _host_launches(n):
    """[(first, count)] of the launches of an n-element host-path call on one device (st_host_chunk_plan / _owner)."""
    return [(first, m) for _, first, m in _capi.host_chunk_map(n, 1)]


def _call_size(per_launch):
    """Elements of a host-path call whose every launch has exactly ``per_launch`` of them."""
    n = per_launch if per_launch <= HOST_CHUNK_MIN else 8 * per_launch
    launches = _host_launches(n)
    assert all(m == per_launch for _, m in launches), (per_launch, launches[:3], launches[-1])
    return n, launches


class _Ref:
    """Expected (distances, MRCA ids) of pair arrays on one tree, cached by key."""

    def __init__(self, parent, dist, full_max=FULL_ORACLE_MAX):
        self.parent, self.dist, self.full_max, self.cache = parent, dist, full_max, {}

    def want(self, dev, key, pairs, launches):
        """Up to full_max pairs: the oracle on every pair.  Beyond: the oracle on a seeded sample of ORACLE_SAMPLE pairs and
        on the first and last LAUNCH_EDGE pairs of every launch; the rest from ``dev``'s explicit-pair path under "walk"."""
        if key in self.cache:
            return self.cache[key]
        n = len(pairs)
        if n <= self.full_max:
            got = oracle_both(self.parent, self.dist, pairs)
        else:
            was = dev.info()["strategy"]
            dev.set_strategy("walk")
            d, m = dev.distances_host(pairs, True, True)
            dev.set_strategy(was)
            rng = np.random.default_rng(n)
            pick = [rng.permutation(n)[:ORACLE_SAMPLE] if n <= 8 * ORACLE_SAMPLE else rng.permutation(np.unique(rng.integers(0, n, 2 * ORACLE_SAMPLE)))[:ORACLE_SAMPLE]]
            for first, count in launches:
                pick.append(np.arange(first, min(first + LAUNCH_EDGE, first + count)))
                pick.append(np.arange(max(first, first + count - LAUNCH_EDGE), first + count))
            pick = np.unique(np.concatenate(pick))
            assert len(pick) >= ORACLE_SAMPLE
            od, om = oracle_both(self.parent, self.dist, pairs[pick])
            assert_bits_equal(d[pick], od, "%s: explicit pairs under walk against the oracle" % (key,))
            assert np.array_equal(m[pick], om), key
            got = (np.array(d), np.array(m))
        self.cache[key] = got
        return got


_REFS = {}


def _ref_for(name, parent, dist, full_max=FULL_ORACLE_MAX):
    """One _Ref per named tree for the whole module: the tests of group A share trees, id lists and expected results."""
    if name not in _REFS:
        _REFS[name] = _Ref(parent, dist, full_max)
    return _REFS[name]


def _mixed_ids(parent, m, seed):
    """m node ids: leaves, 37 internal nodes, the root and two repeated ids, shuffled."""
    rng = np.random.default_rng(seed)
    leaves = _leaves(parent)
    inner = np.setdiff1d(np.arange(len(parent)), leaves)
    root = int(np.flatnonzero(parent < 0)[0])
    k = min(37, len(inner), m // 4)
    ids = np.concatenate([rng.choice(leaves, m - k - 3, replace=len(leaves) < m), rng.choice(inner, k, replace=False), [root]]).astype(np.int64)
    ids = np.concatenate([ids, ids[:2]])
    rng.shuffle(ids)
    assert len(ids) == m
    return ids


# ---- A. kernel form x generator x sink ---------------------------------------------------------------------------

_SEEN = {}      # test name -> set of (kernel, record_bytes, source, sink)


def _kernel(info, opt, n, dist):
    """The kernel one launch of n generated pairs gets, from the handle's reported state and the options this file set
    (host_launch.h:24-28 enqueue_src, launch_canopy.hip:91-115 launch_canopy_t, launch_walk.hip:71 launch_walk).  A launch
    size that leaves the kernel to a threshold this file cannot see from outside fails the test."""
    canopy = info["strategy"] == "canopy"
    if canopy and not dist and opt.get("mrca_ranks", 1) and "ranks" not in info["dropped_tables"] and n >= CANOPY_MIN_PAIRS:
        return "mrca_ranks"
    if canopy and n >= CANOPY_MIN_PAIRS:
        if n < CANOPY_MIN_PAIRS_MAX or opt.get("ladder_min_pairs", 0) > n:
            pytest.fail("a launch of %d pairs lies between the canopy family's thresholds" % n)
        big = info["big_batch_kernel"]
        if big == "canopy_ladder" and (dist or info["record_bytes"] > 512):
            assert n >= LADDER_MIN_PAIRS and opt["ladder_min_pairs"] == 0
            name = "canopy_ladder_joint" if info["ladder_sums"] else "canopy_ladder"
            dyn_min = LADDER_DYNAMIC_MIN // 2 if info["record_bytes"] > 512 else LADDER_DYNAMIC_MIN
            if opt["ladder_dynamic"] and info["record_bytes"] >= 512 and n >= dyn_min:
                name += "+dynamic"
            return name
        if big == "walk_sorted" and dist:
            assert n >= PREFERS_WALK_SORTED_MIN
            return "walk_sorted_ladder"
        if big == "canopy_sorted":
            # (on the host path this holds because of staging: with a's side from the lineage sums the kernel may work on the
            # pinned slots -- launch_policy.h:169 sorted_zero_copy --, otherwise wants_device_stage, :171, moves the chunk through
            # device memory and launches with allow_sorted; either way launch_canopy_t takes the tile-sorted kernel.  Inferred
            # from the policy, like every name here: the library reports no per-launch kernel)
            return "canopy_sorted"
        if big != "canopy":
            assert opt["tile_sort"] == 0      # (what is left then is the predicated kernel)
        return "canopy"
    if dist and n >= WALK_SORTED_MIN_PAIRS and opt["walk_sorted_ready"]:      # (launch_policy.h:187; without its tables k_walk at every size)
        return "walk_sorted_ladder" if opt.get("walk_ladder", 1) else "walk_sorted"
    return "walk"


def _sink(info, dist, mrca, device=False):
    if device:
        return "+".join(s for s, on in (("f64", dist), ("m32", mrca)) if on)
    return "+".join(s for s, on in (("f32", dist), ("m24" if info["host_wire_bytes_out"] == 7 else "m32", mrca)) if on)


_SIZES = {"small": (1500, 100), "mid": (WALK_SORTED_MIN_PAIRS, 1200), "big": (CANOPY_MIN_PAIRS_MAX, 4200)}      # (pairs per launch, ids)


def _sweep(dev, ref, opt, size, seen, seed=1, wires=(1, 0)):
    """Every generator with every sink on one configured handle, launches of _SIZES[size][0] pairs: (a) triangle_host /
    triangle_device over a k-range that starts and ends inside a row, (b) grid_host rectangular and symmetric over element
    ranges that start in mid-row (the symmetric one below the diagonal), (c) quartets_host, (d) knn_host."""
    import torch
    per_launch, m = _SIZES[size]
    n_call, launches = _call_size(per_launch)
    parent = ref.parent
    ids = _mixed_ids(parent, m, seed)
    rec = dev.info()["record_bytes"]

    def note(source, n, dist, mrca, device=False):
        info = dev.info()
        seen.add((_kernel(info, opt, n, dist), rec, source, _sink(info, dist, mrca, device)))

    def sinks():
        """(want_dist, want_mrca) with the options set: both, distances alone, ids alone from the rank table and without."""
        for dist, mrca in ((True, True), (True, False)):
            yield dist, mrca
        for ranks in (1, 0):
            dev.set_option("mrca_ranks", ranks)
            opt["mrca_ranks"] = ranks
            yield False, True
        dev.set_option("mrca_ranks", 1)
        opt["mrca_ranks"] = 1

    def check(got, want, dist, mrca, what):
        if dist:
            assert_bits_equal(got[0], want[0], what)
        if mrca:
            assert np.array_equal(got[1], want[1]), what

    # (a) the triangle: [k0, k0 + n_call) starts at column 5 of a row and ends inside one
    k0 = _T(m // 3) + 5
    while True:
        r_end, c_end = _tri_rc(k0 + n_call - 1, 1)
        if 0 < c_end[0] < r_end[0] - 1:
            break
        k0 += 1
    assert k0 + n_call <= _T(m) and k0 > _T(m // 3)
    tri = _tri_pairs(ids, k0, n_call)
    want_tri = ref.want(dev, ("triangle", size, seed), tri, launches)
    for wire in wires:
        dev.set_option("wire24", wire)
        for dist, mrca in sinks():
            got = dev.triangle_host(ids, k0, n_call, want_dist=dist, want_mrca=mrca)
            check(got, want_tri, dist, mrca, "triangle_host wire24=%d %s" % (wire, opt))
            note("triangle", per_launch, dist, mrca)
    dev.set_option("wire24", 1)
    n_dev = min(per_launch, n_call)
    d_ids = torch.from_numpy(ids).cuda()
    for dist, mrca in sinks():
        out_d = torch.full((n_dev + 8,), -1.0, dtype=torch.float64, device="cuda")
        out_m = torch.full((n_dev + 8,), -7, dtype=torch.int32, device="cuda")
        dev.triangle_device(d_ids.data_ptr(), m, k0, n_dev, out_d.data_ptr() if dist else 0, out_m.data_ptr() if mrca else 0)
        dev.fault_check()
        check((out_d[:n_dev].cpu().numpy(), out_m[:n_dev].cpu().numpy()), (want_tri[0][:n_dev], want_tri[1][:n_dev]), dist, mrca,
              "triangle_device %s" % opt)
        assert out_d[n_dev:].eq(-1.0).all() and out_m[n_dev:].eq(-7).all()
        assert dist or out_d.eq(-1.0).all()
        assert mrca or out_m.eq(-7).all()
        note("triangle", n_dev, dist, mrca, device=True)
    # (b) grids: a rectangle from column 11 of a row on, a symmetric square from (r, 1) with r > 1 on
    nr = m // 2 - m // 40
    rows, cols = ids[:nr], ids[nr:]
    e0 = (nr // 50) * len(cols) + 11
    assert e0 + n_call <= nr * len(cols) and e0 % len(cols) == 11
    want_rect = ref.want(dev, ("rect", size, seed), _grid_pairs(rows, cols, e0, n_call), launches)
    sq = ids[:m // 2]
    r0 = len(sq) // 50 + 2
    s0 = r0 * len(sq) + 1
    assert s0 + n_call <= len(sq) ** 2 and divmod(s0, len(sq)) == (r0, 1) and 1 < r0
    want_sym = ref.want(dev, ("symmetric", size, seed), _grid_pairs(sq, sq, s0, n_call, True), launches)
    for wire in wires:
        dev.set_option("wire24", wire)
        for dist, mrca in sinks():
            got = dev.grid_host(rows, cols, False, e0, n_call, want_dist=dist, want_mrca=mrca)
            check(got, want_rect, dist, mrca, "grid_host wire24=%d %s" % (wire, opt))
            got = dev.grid_host(sq, sq, True, s0, n_call, want_dist=dist, want_mrca=mrca)
            check(got, want_sym, dist, mrca, "grid_host symmetric wire24=%d %s" % (wire, opt))
            note("grid", per_launch, dist, mrca)
    dev.set_option("wire24", 1)
    # (c) quartets: one chunk of the pipe, six pairs each
    nq = -(-per_launch // 6)
    assert nq <= QUARTET_CHUNK
    q = np.random.default_rng(seed + 7).choice(ids, (nq, 4))
    key = ("quartets", size, seed)
    if key not in ref.cache:
        ref.cache[key] = _oracle_quartets(parent, ref.dist, q)
    for ranks in (1, 0):
        dev.set_option("mrca_ranks", ranks)
        opt["mrca_ranks"] = ranks
        assert np.array_equal(dev.quartets_host(q), ref.cache[key]), ("quartets_host", opt)
        info = dev.info()
        if info["strategy"] == "canopy" and 6 * nq >= CANOPY_MIN_PAIRS:
            assert 6 * nq >= CANOPY_MIN_PAIRS_MAX      # (host_quartets.h: quartets_host_run: the canopy route for certain)
            seen.add((_kernel(info, opt, 6 * nq, False), rec, "quartet", "m32"))
        else:
            seen.add(("quartets_walk", rec, "quartet", "topology"))
    dev.set_option("mrca_ranks", 1)
    opt["mrca_ranks"] = 1
    # (d) k nearest: one block of rows, the float32 sink
    nk = {"small": 20, "mid": 300, "big": 600}[size]
    queries = ids[:nk]
    cands = ids[nk:nk + -(-per_launch // nk)]
    n_knn = nk * len(cands)
    assert per_launch <= n_knn <= KNN_BLOCK_ELEMS and len(cands) > 16
    want_d, _ = ref.want(dev, ("knn", size, seed), _grid_pairs(queries, cands, 0, n_knn), [(0, n_knn)])
    for skip in (0, 1):
        idx, d = dev.knn_host(queries, cands, 7, skip_self=skip)
        want_idx, want_kd = _knn_want(want_d.reshape(nk, len(cands)), queries, cands, 7, skip)
        assert np.array_equal(idx, want_idx), ("knn_host", skip, opt)
        assert_bits_equal(d, want_kd, "knn_host skip_self=%d %s" % (skip, opt))
    seen.add((_kernel(dev.info(), opt, n_knn, True), rec, "grid", "f32 knn"))


def _knn_want(rows64, queries, cands, k, skip_self):
    """(index, distance) of the k nearest candidates per row of the float64 (widened float32) distance matrix: numpy's
    stable argsort of the float32 row -- NaN last, -0.0 == +0.0, index order on ties --, candidates equal to the query left
    out with skip_self; -1 / NaN where fewer than k remain."""
    n_q, n_c = rows64.shape
    idx = np.full((n_q, k), -1, np.int64)
    dist = np.full((n_q, k), np.nan)
    for i in range(n_q):
        order = np.argsort(rows64[i].astype(np.float32), kind="stable")
        if skip_self:
            order = order[cands[order] != queries[i]]
        order = order[:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = rows64[i][order]
    return idx, dist


def _assert_knn_dist(got, want, what):
    """Distances bit for bit; a NaN where a NaN is expected (its sign and payload are nobody's contract)."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert_bits_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def _set(dev, opt, **options):
    for k, v in options.items():
        dev.set_option(k, v)
        opt[k] = v


def test_a_predicated_kernel_on_short_records():
    """k_canopy_ilp<1 / 3 / 7, 1, Src> -- the plain form, which generators take on trees whose explicit pairs take the
    four-byte a side (launch_canopy.hip:109-114) -- on 16-, 32- and 64-byte records (balanced trees of 2^16 ... 2^18 leaves
    have 32- and 64-byte records; the 16-byte ones come from 2^13 leaves).  Every pair against the oracle up to
    2^20 pairs, the 8 x 524288-pair calls by sample (see _Ref.want)."""
    seen = _SEEN.setdefault("predicated short", set())
    records = set()
    for name, (parent, dist) in (("balanced 2^13", synth.balanced_tree(13)), ("balanced 2^16", synth.balanced_tree(16)),
                                 ("balanced 2^18", synth.balanced_tree(18)), ("complete 50000", synth.complete_tree(50_000, seed=2))):
        dev = _capi.DeviceTree(parent, dist)
        info = dev.info()
        assert info["strategy"] == "canopy" and info["big_batch_kernel"] == "canopy" and info["a_side_bytes"] == 4, (name, info)
        records.add(info["record_bytes"])
        _sweep(dev, _Ref(parent, dist), {"tile_sort": None}, "big", seen, seed=len(parent))
        dev.close()
    assert records == {16, 32, 64}, records


def _cap63_tree():
    return synth.skewed_tree(np.random.default_rng(61), 54_000, 0.95)      # (test_ladder_kernel_joint_form_keeps_the_bits: "cap63")


@pytest.mark.parametrize("which", ["nj", "cap63"])
def test_a_predicated_kernel_on_long_records(which, nj_arrays):
    """k_canopy_ilp<31 / 63, 1, Src> on 256- and 512-byte records.  By sample (see _Ref.want)."""
    parent, dist = (nj_arrays[0], nj_arrays[1]) if which == "nj" else _cap63_tree()
    dev = _capi.DeviceTree(parent, dist, strategy="canopy")
    opt = {}
    _set(dev, opt, tile_sort=0, ladder_scalar=0, prefer_walk_sorted=0)
    info = dev.info()
    assert info["big_batch_kernel"] == "canopy" and info["record_bytes"] == {"nj": 256, "cap63": 512}[which], info
    _sweep(dev, _ref_for(which, parent, dist), opt, "big", _SEEN.setdefault("predicated " + which, set()), seed=9)
    dev.close()


def _skewed_candidates():
    rng = np.random.default_rng(404)      # (test_gpu_parity.py::test_lineage_sum_mode_of_the_deep_kernel's small deep trees)
    for n, skew in ((30000, 0.97), (9000, 0.995), (11000, 0.9), (16000, 0.9)):
        yield synth.skewed_tree(rng, n, skew)


def test_a_tile_sorted_canopy_kernel():
    """launch_canopy_sorted<1 / 3 / 7> as the handle is built (a's side from the lineage sums, the kernel works on the pinned
    slots) and with lineage_sums = 0 (the other scratch layout; staged through device memory).  By sample."""
    for parent, dist in _skewed_candidates():
        dev = _capi.DeviceTree(parent, dist)
        opt = {}
        _set(dev, opt, tile_sort=1, ladder_scalar=0, prefer_walk_sorted=0)
        if dev.info()["big_batch_kernel"] == "canopy_sorted":
            break
        dev.close()
    else:
        pytest.fail("no small deep tree runs the tile-sorted canopy kernel")
    seen = _SEEN.setdefault("canopy_sorted", set())
    ref = _Ref(parent, dist)
    for sums in (1, 0):
        _set(dev, opt, lineage_sums=sums)
        assert dev.info()["big_batch_kernel"] == "canopy_sorted"
        _sweep(dev, ref, opt, "big", seen, seed=5)
    dev.close()


def _ladder_tree(which, ml_arrays, nj_arrays):
    if which == "ml":
        return ml_arrays[0], ml_arrays[1]
    if which == "nj":
        return nj_arrays[0], nj_arrays[1]
    if which == "cap63":
        return _cap63_tree()
    return synth.skewed_tree(np.random.default_rng(5), 1_000_000, 0.9)      # (bench.py's walk_only_tree leg: 1 KB records)


@pytest.mark.parametrize("which", ["ml", "nj", "cap63", "cap127"])
def test_a_scalar_ladder_kernel(which, ml_arrays, nj_arrays):
    """k_canopy_ladder<15 / 31 / 63 / 0, Src, joint> with ladder_sums and ladder_dynamic 0 and 1; the dynamic deal (records
    of 512 bytes and more, launches of 2^22 pairs, 2^21 on 1 KB records) through a 5800 x 5800 symmetric grid on the host
    path -- 8 x 2^22 elements of it, eight launches of 2^22 by st_host_chunk_plan -- and one triangle_device launch of 2^22.  By sample (see _Ref.want);
    on the 1e6-leaf tree every call beyond 2^17 pairs."""
    import torch
    parent, dist = _ladder_tree(which, ml_arrays, nj_arrays)
    dev = _capi.DeviceTree(parent, dist, strategy="canopy")
    info = dev.info()
    assert info["record_bytes"] == {"ml": 128, "nj": 256, "cap63": 512}.get(which, info["record_bytes"])
    if which == "cap127" and info["record_bytes"] != 1024:
        pytest.skip("this shape did not need 1 KB records (record_bytes %d)" % info["record_bytes"])
    rec = info["record_bytes"]
    opt = {}
    _set(dev, opt, tile_sort=0, ladder_scalar=1, ladder_min_pairs=0, prefer_walk_sorted=0, batch_probe=0, ladder_dynamic=0)
    assert dev.info()["big_batch_kernel"] == "canopy_ladder"
    seen = _SEEN.setdefault("ladder " + which, set())
    ref = _ref_for(which, parent, dist, 1 << 17 if which == "cap127" else FULL_ORACLE_MAX)
    for sums in (1, 0):
        for dynamic in (0, 1):
            _set(dev, opt, ladder_sums=sums, ladder_dynamic=dynamic)
            if which != "cap127":      # (the 1e6-leaf tree's lineage sums exceed the canopy family's limit: the climbing form runs)
                assert dev.info()["ladder_sums"] == sums
            _sweep(dev, ref, opt, "big", seen, seed=9)
    if rec >= 512:
        dyn_min = LADDER_DYNAMIC_MIN // 2 if rec > 512 else LADDER_DYNAMIC_MIN
        ids = _mixed_ids(parent, 5800, 77)
        n = 8 * LADDER_DYNAMIC_MIN      # (the whole square would end in a ninth launch of 85,568 elements, below every canopy threshold)
        g0 = 7 * len(ids) + 3           # from (7, 3), below the diagonal in mid-row
        launches = _host_launches(n)
        assert g0 + n <= len(ids) ** 2 and len(launches) == 8 and all(c == HOST_CHUNK_MAX >= dyn_min for _, c in launches)
        want = ref.want(dev, "5800 x 5800", _grid_pairs(ids, ids, g0, n, True), launches)
        m_ids = _mixed_ids(parent, 4200, 9)
        k0 = _T(1400) + 5
        n_dev = LADDER_DYNAMIC_MIN
        want_tri = ref.want(dev, "triangle 2^22", _tri_pairs(m_ids, k0, n_dev), [(0, n_dev)])
        d_ids = torch.from_numpy(m_ids).cuda()
        for sums in (1, 0):
            _set(dev, opt, ladder_sums=sums, ladder_dynamic=1)
            for mrca, wire in ((True, 1), (True, 0), (False, 1)):
                dev.set_option("wire24", wire)
                d, m = dev.grid_host(ids, ids, True, g0, n, want_dist=True, want_mrca=mrca)
                assert_bits_equal(d, want[0], "5800 x 5800 symmetric, dynamic deal, sums=%d wire24=%d" % (sums, wire))
                assert not mrca or np.array_equal(m, want[1])
                name = _kernel(dev.info(), opt, HOST_CHUNK_MAX, True)
                assert name.endswith("+dynamic"), name
                seen.add((name, rec, "grid", _sink(dev.info(), True, mrca)))
                dev.set_option("wire24", 1)
                out_d = torch.full((n_dev + 8,), -1.0, dtype=torch.float64, device="cuda")
                out_m = torch.full((n_dev + 8,), -7, dtype=torch.int32, device="cuda")
                dev.triangle_device(d_ids.data_ptr(), len(m_ids), k0, n_dev, out_d.data_ptr(), out_m.data_ptr() if mrca else 0)
                dev.fault_check()
                assert_bits_equal(out_d[:n_dev].cpu().numpy(), want_tri[0], "triangle_device 2^22, dynamic deal, sums=%d" % sums)
                assert not mrca or np.array_equal(out_m[:n_dev].cpu().numpy(), want_tri[1])
                assert out_d[n_dev:].eq(-1.0).all() and out_m[n_dev:].eq(-7).all()
                seen.add((_kernel(dev.info(), opt, n_dev, True), rec, "triangle", _sink(dev.info(), True, mrca, device=True)))
    dev.close()


def test_a_walk_family(ml_arrays):
    """k_walk (small launches), k_walk_sorted with and without the crown ladder (launches of 262144 under "walk"; launches of
    524288 under "canopy" with prefer_walk_sorted), a tree only the walk family serves, and handles whose table budget
    dropped rec_i and the canopy.  Up to 2^20 pairs every pair against the oracle, beyond by sample."""
    parent, dist, _ = ml_arrays
    ref = _ref_for("ml", parent, dist)
    seen = _SEEN.setdefault("walk family", set())
    dev = _capi.DeviceTree(parent, dist)
    ready = dev.info()["lineage_entries"] > len(parent) and not set(dev.info()["dropped_tables"]) & {"lineage_len", "lineage_sum", "tree_rmq"}
    assert ready, dev.info()      # (launch_policy.h:187 walk_sorted_ready)
    opt = {"walk_sorted_ready": True}
    dev.set_strategy("walk")
    _sweep(dev, ref, opt, "small", seen)
    for wl in (0, 1):
        _set(dev, opt, walk_ladder=wl)
        _sweep(dev, ref, opt, "mid", seen)
    dev.set_strategy("canopy")
    _set(dev, opt, tile_sort=0, ladder_scalar=0, prefer_walk_sorted=1, walk_ladder=1)
    assert dev.info()["big_batch_kernel"] == "walk_sorted", dev.info()
    _sweep(dev, ref, opt, "big", seen, seed=9)
    dev.close()
    for mb, dropped in ((16, "rec_i"), (8, "canopy")):
        dev = _capi.DeviceTree(parent, dist, table_mb=mb)
        info = dev.info()
        assert dropped in info["dropped_tables"], info
        opt = {"walk_sorted_ready": not set(info["dropped_tables"]) & {"lineage_len", "lineage_sum", "tree_rmq"}, "tile_sort": None}
        if info["strategy"] == "canopy":
            _set(dev, opt, tile_sort=0, ladder_scalar=0, prefer_walk_sorted=0)
            assert dev.info()["big_batch_kernel"] == "canopy"
            _sweep(dev, ref, opt, "big", _SEEN.setdefault("table_mb=%d" % mb, set()), seed=9)
        else:
            _sweep(dev, ref, opt, "small", _SEEN.setdefault("table_mb=%d" % mb, set()))
            _sweep(dev, ref, opt, "mid", _SEEN["table_mb=%d" % mb])
        dev.close()
    # a tree the canopy family refuses (test_walk_only_tree_with_sparse_table_and_lineage_sums)
    wparent, wdist = synth.skewed_tree(np.random.default_rng(7), 120_000, 0.97)
    dev = _capi.DeviceTree(wparent, wdist)
    info = dev.info()
    assert info["strategy"] == "walk" and info["lineage_entries"] > len(wparent), info
    wref = _Ref(wparent, wdist, full_max=1 << 16)
    wseen = _SEEN.setdefault("walk only", set())
    opt = {"walk_sorted_ready": True}
    _sweep(dev, wref, opt, "small", wseen)
    _sweep(dev, wref, opt, "mid", wseen)
    dev.close()


def test_a_cells_seen():
    """The (kernel, record_bytes) x source/sink cells the group's tests reached, literally: a change of policy that takes a
    generator away from a kernel form fails here.  Needs the tests above in the same session.  (sinks: f32 / m24 / m32 the
    host path's wire, f64 / m32 device buffers, knn-f32 the distance block of st_knn_host; record_bytes 0: no canopy tables)"""
    if not _SEEN:
        pytest.fail("group A's tests did not run in this session: run the whole file")
    got = {}
    for name, cells in _SEEN.items():
        for kernel, rec, source, sink in cells:
            got.setdefault(name, {}).setdefault((kernel, rec), set()).add(source + "/" + sink.replace("f32 knn", "knn-f32"))
    got = {name: {key: " ".join(sorted(v)) for key, v in g.items()} for name, g in got.items()}
    want = dict(_EXPECTED_CELLS)
    if "ladder cap127" not in got:      # (skipped above: the shape did not need 1 KB records)
        del want["ladder cap127"]
    assert got == want


_EXPECTED_CELLS = {
    'predicated short': {
        ('canopy', 16): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('canopy', 32): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('canopy', 64): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 16): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 32): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 64): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'predicated nj': {
        ('canopy', 256): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 256): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'predicated cap63': {
        ('canopy', 512): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 512): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'canopy_sorted': {
        ('canopy_sorted', 16): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 16): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'ladder ml': {
        ('canopy', 128): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('canopy_ladder', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('canopy_ladder_joint', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('mrca_ranks', 128): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'ladder nj': {
        ('canopy', 256): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('canopy_ladder', 256): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('canopy_ladder_joint', 256): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('mrca_ranks', 256): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'ladder cap63': {
        ('canopy', 512): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('canopy_ladder', 512): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('canopy_ladder+dynamic', 512): 'grid/f32 grid/f32+m24 grid/f32+m32 triangle/f64 triangle/f64+m32',
        ('canopy_ladder_joint', 512): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('canopy_ladder_joint+dynamic', 512): 'grid/f32 grid/f32+m24 grid/f32+m32 triangle/f64 triangle/f64+m32',
        ('mrca_ranks', 512): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'ladder cap127': {
        ('canopy_ladder', 1024): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('canopy_ladder+dynamic', 1024): 'grid/f32 grid/f32+m24 grid/f32+m32 triangle/f64 triangle/f64+m32',
        ('mrca_ranks', 1024): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'walk family': {
        ('canopy', 128): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 128): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
        ('quartets_walk', 128): 'quartet/topology',
        ('walk', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('walk_sorted', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
        ('walk_sorted_ladder', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
    },
    'table_mb=16': {
        ('canopy', 128): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 quartet/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('mrca_ranks', 128): 'grid/m24 grid/m32 quartet/m32 triangle/m24 triangle/m32',
    },
    'table_mb=8': {
        ('quartets_walk', 0): 'quartet/topology',
        ('walk', 0): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
    },
    'walk only': {
        ('quartets_walk', 0): 'quartet/topology',
        ('walk', 0): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 grid/m24 grid/m32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32 triangle/m24 triangle/m32',
        ('walk_sorted_ladder', 0): 'grid/f32 grid/f32+m24 grid/f32+m32 grid/knn-f32 triangle/f32 triangle/f32+m24 triangle/f32+m32 triangle/f64 triangle/f64+m32',
    },
}


# ---- B. triangle and grid index arithmetic against an independent reference ----------------------------------------

def _uncorrected_row(k):
    """device_common.h:81 without its two corrections, in numpy's IEEE float64."""
    return np.floor((1.0 + np.sqrt(1.0 + 8.0 * np.asarray(k, np.int64).astype(np.float64))) * 0.5).astype(np.int64)


def _boundary_rows(lo, hi):
    """Rows r in [lo, hi) where the uncorrected formula is one too large at k = T(r) - 1, and where it is one too small at
    k = T(r).  With a correctly rounded sqrt the first kind is every row from about 9.5e7 on (sqrt((2r-1)^2 - 8) rounds to
    2r - 1 once 4 / (2r - 1) is below half an ulp) and the second kind does not occur up to the ABI's cap; a sqrt one ulp
    low would be one too small at EVERY T(r), which is why the ranges below sit on those k at every scale."""
    r = np.arange(lo, hi, dtype=np.int64)
    t = r * (r - 1) // 2
    return r[_uncorrected_row(t - 1) == r], r[_uncorrected_row(t) == r - 1]


def _boundary_ranges(r, count):
    """k-ranges that end exactly on / start exactly on k = T(r) - 1 and k = T(r)."""
    for k in (_T(r) - 1, _T(r)):
        yield k - count + 1, count
        yield k, count


def test_b_triangle_row_boundaries():
    """triangle_host / triangle_device over k-ranges that start and end exactly on T(r) - 1 and T(r) for r near 2^12, 2^16
    and 10^5, on 100,000 distinct leaves (every row and column is its own id).  Every pair against the oracle."""
    import torch
    m = 100_000
    parent, dist = synth.complete_tree(m, seed=44)
    ids = _leaves(parent)
    assert len(ids) == m and len(np.unique(ids)) == m
    dev = _capi.DeviceTree(parent, dist)
    d_ids = torch.from_numpy(ids).cuda()
    count = 20_000
    for scale in (1 << 12, 1 << 16, m - 10):
        too_large, too_small = _boundary_rows(scale - 64, min(scale + 64, m))
        for r in sorted({scale, *too_large[:1].tolist(), *too_small[:1].tolist()}):
            for k0, c in _boundary_ranges(r, count):
                assert 0 <= k0 and k0 + c <= _T(m)
                pairs = _tri_pairs(ids, k0, c)
                want_d, want_m = oracle_both(parent, dist, pairs)
                d, mm = dev.triangle_host(ids, k0, c, want_dist=True, want_mrca=True)
                assert_bits_equal(d, want_d, "triangle_host r=%d k0=%d" % (r, k0))
                assert np.array_equal(mm, want_m), (r, k0)
                out_d = torch.empty(c, dtype=torch.float64, device="cuda")
                out_m = torch.empty(c, dtype=torch.int32, device="cuda")
                dev.triangle_device(d_ids.data_ptr(), m, k0, c, out_d.data_ptr(), out_m.data_ptr())
                dev.fault_check()
                assert_bits_equal(out_d.cpu().numpy(), want_d, "triangle_device r=%d k0=%d" % (r, k0))
                assert np.array_equal(out_m.cpu().numpy(), want_m), (r, k0)
    dev.close()


def test_b_triangle_device_beyond_2_53():
    """k beyond 2^53, where (double)k is inexact, over a device-resident list of 1.5e8 ids (1.2 GB, built with torch; the
    pairs are never materialised): the end of the triangle, ranges that start and end exactly on T(r) - 1 for a row where
    the uncorrected formula is one too large there (found on the CPU) and on T(r), across 2^53, and with id_stride = 2.
    ids[i] = leaf (i mod 2^16) of a balanced tree: neighbouring rows and columns are different leaves.  The list sits
    between guard entries holding another leaf, so a row or column that is off by one past either end reads a wrong id,
    not foreign memory.  Every pair against the oracle."""
    import torch
    m = 150_000_000
    guard = 4
    parent, dist = synth.balanced_tree(16)
    n_leaves = 1 << 16
    dev = _capi.DeviceTree(parent, dist)
    buf = torch.empty(m + 2 * guard, dtype=torch.int64, device="cuda")
    buf[:guard] = 2 * 12345
    buf[m + guard:] = 2 * 23456
    torch.remainder(torch.arange(m, dtype=torch.int64, device="cuda"), n_leaves, out=buf[guard:m + guard])
    buf[guard:m + guard] *= 2      # (leaf j has id 2 j)
    d_ids = buf.data_ptr() + 8 * guard
    total = _T(m)
    assert total > 2 ** 53 and m <= TRIANGLE_MAX_M
    too_large, too_small = _boundary_rows(m - 200_000, m)
    assert len(too_large) > 0      # (the `row--` correction is load-bearing here)
    r1 = int(too_large[len(too_large) // 2])
    r2 = int(too_small[0]) if len(too_small) else m - 12_345
    assert 8 * _T(r2) > 2 ** 53
    count = 200_000
    ranges = [(total - count, count, 1), (2 ** 53 - count // 2, count, 1)]
    ranges += [(k0, c, 1) for k0, c in _boundary_ranges(r1, count)] + [(k0, c, 1) for k0, c in _boundary_ranges(r2, count)]
    m2 = m // 2
    ranges += [(_T(m2) - count, count, 2), (_T(m2 - 77_777) - 5, count, 2)]
    out_d = torch.empty(count + 8, dtype=torch.float64, device="cuda")
    out_m = torch.empty(count + 8, dtype=torch.int32, device="cuda")
    for k0, c, stride in ranges:
        rows, cols = _tri_rc(k0, c)
        assert rows.max() < (m if stride == 1 else m2)
        pairs = np.stack([(cols * stride) % n_leaves * 2, (rows * stride) % n_leaves * 2], 1)
        want_d, want_m = oracle_both(parent, dist, pairs)
        out_d.fill_(-1.0)
        out_m.fill_(-7)
        dev.triangle_device(d_ids, m if stride == 1 else m2, k0, c, out_d.data_ptr(), out_m.data_ptr(), id_stride=stride)
        dev.fault_check()
        assert_bits_equal(out_d[:c].cpu().numpy(), want_d, "k0=%d stride=%d" % (k0, stride))
        assert np.array_equal(out_m[:c].cpu().numpy(), want_m), (k0, stride)
        assert out_d[c:].eq(-1.0).all() and out_m[c:].eq(-7).all()
    with pytest.raises(ValueError):
        dev.triangle_device(d_ids, m, total - 10, 11, out_d.data_ptr(), out_m.data_ptr())
    dev.close()


def test_b_grid_edges():
    """SrcGrid: one column, one row, a 1 x 1 symmetric grid; a rectangle of more than 2^32 elements addressed through e_begin
    at its end and across 2^31 and 2^32; a symmetric element range that starts below the diagonal.  Every pair against the
    oracle."""
    parent, dist = synth.complete_tree(100_000, seed=44)
    leaves = _leaves(parent)
    dev = _capi.DeviceTree(parent, dist)
    rng = np.random.default_rng(12)

    def run(rows, cols, symmetric, e0, count, what):
        pairs = _grid_pairs(rows, cols, e0, count, symmetric)
        want_d, want_m = oracle_both(parent, dist, pairs)
        d, m = dev.grid_host(rows, cols, symmetric, e0, count, want_dist=True, want_mrca=True)
        assert_bits_equal(d, want_d, what)
        assert np.array_equal(m, want_m), what
        assert np.array_equal(dev.grid_host(rows, cols, symmetric, e0, count, want_dist=False, want_mrca=True)[1], want_m), what

    ids = rng.choice(leaves, 5000, replace=False)
    ids[3] = int(parent[ids[4]])
    run(ids[:700], ids[:1], False, 0, 700, "one column")
    run(ids[:700], ids[:1], False, 13, 600, "one column, a range")
    run(ids[:1], ids[:900], False, 0, 900, "one row")
    run(ids[5:6], ids[5:6], True, 0, 1, "1 x 1 symmetric")
    run(ids[3:4], ids[3:4], True, 0, 1, "1 x 1 symmetric, an internal node")
    rows, cols = rng.choice(leaves, 70_000, replace=False), rng.choice(leaves, 70_000, replace=False)
    total = len(rows) * len(cols)
    assert total > 2 ** 32
    for e0 in (total - 100_000, 2 ** 31 - 50_000, 2 ** 32 - 50_000):
        run(rows, cols, False, e0, 100_000, "70000 x 70000 from element %d" % e0)
    with pytest.raises(ValueError):
        dev.grid_host(rows, cols, False, total - 10, 11)
    e0 = 3000 * 5000 + 17
    assert divmod(e0, 5000) == (3000, 17)
    run(ids, ids, True, e0, 60_000, "symmetric from (3000, 17)")
    dev.close()


# ---- C. quartets ---------------------------------------------------------------------------------------------------

def test_c_quartet_chunks_and_routes(ml_arrays):
    """st_quartets_host against OracleTree.quartets, every quartet: one quartet, exactly one chunk, two chunks and a
    one-quartet tail (the tail goes to launch_quartets_walk, the full chunks through the canopy route: one call mixes
    both), the same under "walk", a strided view, four equal ids, an id out of range in the tail chunk."""
    parent, dist, leaf_ids = ml_arrays
    dev = _capi.DeviceTree(parent, dist)
    assert dev.info()["strategy"] == "canopy"
    rng = np.random.default_rng(21)
    n = 2 * QUARTET_CHUNK + 1
    big = rng.choice(leaf_ids, (n, 4))
    big[1000:1200] = rng.integers(0, len(parent), (200, 4))      # internal nodes
    big[5] = big[5, 0]                                          # four equal ids
    big[-1] = rng.integers(0, len(parent), 4)
    want = _oracle_quartets(parent, dist, big)
    # host_quartets.h: quartets_host_run: a chunk of m quartets takes the canopy route iff 6 m >= canopy_min_pairs(t).  (By the
    # restated thresholds only: no reported state exposes the route of a chunk, and both routes are defined to give the same
    # topologies, so forcing the tail through either is an equivalent mutant -- LAB_NOTES.md)
    assert 6 * 1 < CANOPY_MIN_PAIRS and 6 * QUARTET_CHUNK >= CANOPY_MIN_PAIRS_MAX and n % QUARTET_CHUNK == 1
    for strategy in ("canopy", "walk"):
        dev.set_strategy(strategy)
        for ranks in (1, 0):
            dev.set_option("mrca_ranks", ranks)
            assert np.array_equal(dev.quartets_host(big), want), (strategy, ranks, "two chunks and one quartet")
            assert np.array_equal(dev.quartets_host(big[:QUARTET_CHUNK]), want[:QUARTET_CHUNK]), (strategy, ranks, "one chunk")
        assert np.array_equal(dev.quartets_host(big[-1:]), want[-1:]), strategy
        assert np.array_equal(dev.quartets_host(big[5:6]), want[5:6]) and sorted(want[5]) == sorted(big[5]), strategy
        wide = np.full((2 * 7001, 12), -1, dtype=np.int64)
        wide[::2, 1:12:3] = big[:7001]
        view = wide[::2, 1:12:3]
        assert view.shape == (7001, 4) and view.strides == (2 * 12 * 8, 3 * 8)
        assert np.array_equal(dev.quartets_host(view), want[:7001]), strategy
        bad = big.copy()
        bad[-1, 2] = len(parent) + 11
        with pytest.raises(InvalidNodeError) as err:
            dev.quartets_host(bad)
        assert err.value.node_id == len(parent) + 11
        assert np.array_equal(dev.quartets_host(big[:3000]), want[:3000]), strategy      # (clean after the error)
    dev.close()


# ---- D. k nearest --------------------------------------------------------------------------------------------------

def _knn_tree(values, zero=0.0):
    """A balanced tree of 2048 leaves whose every branch has length ``zero`` except leaf j + 1, which gets values[j]: the
    distance from leaf 0 (or any internal node) to leaf j + 1 is values[j] itself in float32."""
    parent, dist = synth.balanced_tree(11)
    dist = np.full(len(dist), np.float32(zero), dtype=np.float32)
    dist[parent < 0] = np.float32(-1.0)
    leaves = np.arange(0, len(parent), 2, dtype=np.int64)
    dist[leaves[1:1 + len(values)]] = np.asarray(values, dtype=np.float32)
    return parent, dist, leaves


def _knn_check(dev, O, queries, cands, k, skip_self, what):
    rows = O.distances(_grid_pairs(queries, cands, 0, len(queries) * len(cands))).reshape(len(queries), len(cands))
    want_idx, want_d = _knn_want(rows, queries, cands, k, skip_self)
    idx, d = dev.knn_host(queries, cands, k, skip_self=skip_self)
    assert np.array_equal(idx, want_idx), (what, idx, want_idx)
    _assert_knn_dist(d, want_d, what)
    return idx, d


def test_d_knn_key_orders_special_values_like_argsort():
    """Negative distances, -inf, +inf, NaN of either sign and +-0 in one row: np.argsort(kind="stable") of the float32 row,
    NaN last, index order on ties.  Leaf and internal-node queries.  Every distance from the oracle."""
    neg_nan = np.frombuffer(np.uint32(0xFFC00000).tobytes(), dtype=np.float32)[0]
    special = [3.0, -1.5, np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-42, -1e-42, -2.5, neg_nan, -3e38, 3e38, 0.0, -0.0, -1.5, np.inf,
               -np.inf, 2.0, -2.0]
    for zero in (0.0, -0.0):
        parent, dist, leaves = _knn_tree(special * 3, zero)
        O = OracleTree(parent, dist)
        dev = _capi.DeviceTree(parent, dist)
        cands = leaves[1:1 + 3 * len(special)]
        rng = np.random.default_rng(3)
        cands = cands[rng.permutation(len(cands))]
        inner = np.array([1, 3, 1023, int(np.flatnonzero(parent < 0)[0])], dtype=np.int64)
        queries = np.concatenate([leaves[:1], leaves[200:203], inner])
        row = O.distances(_grid_pairs(queries[:1], cands, 0, len(cands))).astype(np.float32)
        assert np.isnan(row).sum() == 6 and np.isneginf(row).sum() == 6 and np.isposinf(row).sum() == 6 and (row < 0).sum() >= 15
        assert (row == 0).sum() == 12
        for k in (1, 7, len(cands) - 6, len(cands)):
            idx, d = _knn_check(dev, O, queries, cands, k, 0, "special values zero=%r k=%d" % (zero, k))
        assert np.isnan(d[:, -6:]).all() and (idx[:, -6:] >= 0).all() and not np.isnan(d[:, :-6]).any()      # (NaN last, and found)
        dev.close()


def test_d_knn_ties_across_lanes_and_waves_and_k_256():
    """Groups of equal distances placed so that one tie straddles candidates 63 | 64 (a wave boundary of k_knn_select's first
    pass), 255 | 256 (its 256-lane stride: the same lane's first and second candidate) and 1023 | 1024; n_cands = 63 ... 1025;
    k = 1, 255, 256 on the device, and the facade's host sort at k = 257 with the same leading 256.  Every distance from
    the oracle."""
    rng = np.random.default_rng(8)
    values = np.round(1.0 + rng.uniform(0.0, 4.0, 1025), 4)
    values[[61, 62, 63, 64, 65, 66]] = 0.5            # the smallest, across the wave boundary
    values[[254, 255, 256, 257]] = 0.5                # ... and across the stride
    values[[1022, 1023, 1024]] = 0.5
    values[[0, 1, 2, 318, 319, 320]] = 0.75           # lanes 62-64 of the second pass tie with the first candidates
    values[[100, 356, 612, 868]] = 0.25               # one lane, its four candidates
    parent, dist, leaves = _knn_tree(values)
    O = OracleTree(parent, dist)
    T = SuchTree((parent, dist))
    dev = T._device_tree()
    all_cands = leaves[1:1026]
    queries = np.array([leaves[0], 1, leaves[1500]], dtype=np.int64)
    for n_c in (63, 64, 65, 255, 256, 257, 1025):
        cands = all_cands[:n_c]
        for k in (1, 255, 256):
            idx, d = _knn_check(dev, O, queries, cands, k, 0, "n_cands=%d k=%d" % (n_c, k))
            if k == 256 and n_c >= 257:
                assert (idx >= 0).all() and np.all(np.diff(d, axis=1) >= 0)
                tie = d[0] == 0.5
                assert np.all(np.diff(idx[0][tie]) > 0) and tie.sum() == (values[:n_c] == 0.5).sum()      # (index order inside a tie)
        if n_c >= 257:
            host = T.nearest_neighbors(int(queries[0]), k=KNN_MAX_K + 1, from_nodes=[int(c) for c in cands])      # (the host sort)
            assert len(host) == KNN_MAX_K + 1
            assert [x for x, _ in host[:KNN_MAX_K]] == cands[idx[0]].tolist()
            assert_bits_equal(np.array([x for _, x in host[:KNN_MAX_K]]), d[0], "host sort at k = 257, n_cands=%d" % n_c)


def test_d_knn_skip_self_and_repeated_queries():
    """n_cands == k with skip_self and the query among the candidates (the last slot is -1 / NaN), the query listed three
    times among the candidates with and without skip_self, internal-node queries.  Every distance from the oracle."""
    rng = np.random.default_rng(9)
    parent, dist = synth.random_binary_tree(3000, seed=12)
    leaves = _leaves(parent)
    O = OracleTree(parent, dist)
    dev = _capi.DeviceTree(parent, dist)
    cands = rng.choice(leaves, 64, replace=False)
    queries = np.array([cands[10], cands[63], cands[0]], dtype=np.int64)
    idx, d = _knn_check(dev, O, queries, cands, 64, 1, "n_cands == k, skip_self")
    assert (idx[:, -1] == -1).all() and np.isnan(d[:, -1]).all() and (idx[:, :-1] >= 0).all()
    for i, q in enumerate(queries):
        assert q not in cands[idx[i, :-1]]
    idx, d = _knn_check(dev, O, queries, cands, 64, 0, "n_cands == k")
    assert (cands[idx[:, 0]] == queries).all() and (d[:, 0] == 0).all()
    thrice = np.concatenate([cands[:20], queries[:1], cands[20:40], queries[:1], queries[:1], cands[40:]])
    assert (thrice == queries[0]).sum() == 4      # (it was a candidate already)
    idx, d = _knn_check(dev, O, queries, thrice, 8, 0, "the query four times among the candidates")
    assert (thrice[idx[0, :4]] == queries[0]).all() and np.all(np.diff(idx[0, :4]) > 0) and (d[0, :4] == 0).all()
    idx, d = _knn_check(dev, O, queries, thrice, 8, 1, "the query four times among the candidates, skip_self")
    assert queries[0] not in thrice[idx[0]]
    idx, d = _knn_check(dev, O, queries, thrice, len(thrice), 1, "... k = n_cands")
    assert (idx[0, -4:] == -1).all() and (idx[0, :-4] >= 0).all() and (idx[1, -1] == -1) and (idx[1, -2] >= 0)
    inner = np.setdiff1d(np.arange(len(parent)), leaves)
    _knn_check(dev, O, rng.choice(inner, 40), np.concatenate([cands, inner[:30]]), 12, 1, "internal-node queries")
    dev.close()


def test_d_knn_row_blocks(ml_arrays):
    """st_knn_host beyond 2^26 distances: three row blocks, the last one short.  Rows at the block edges and a seeded dozen
    more against the oracle (every distance of those rows), ids and distances, with the index tie rule; skip_self with
    leaf queries, so a block that read another block's queries would report the query itself at distance 0."""
    parent, dist, leaf_ids = ml_arrays
    dev = _capi.DeviceTree(parent, dist)
    O = OracleTree(parent, dist)
    cands = leaf_ids
    rows_per_block = max(1, KNN_BLOCK_ELEMS // len(cands))      # host_misc.h: knn_host_run (n_queries is larger)
    n_q = 2 * rows_per_block + 17
    blocks = -(-n_q // rows_per_block)
    assert n_q * len(cands) > KNN_BLOCK_ELEMS and blocks == 3 and n_q % rows_per_block == 17
    rng = np.random.default_rng(14)
    queries = rng.choice(leaf_ids, n_q, replace=False)
    k = 5
    idx, d = dev.knn_host(queries, cands, k, skip_self=True)
    assert idx.shape == (n_q, k) and (idx >= 0).all()
    assert not (cands[idx] == queries[:, None]).any()      # (no query is its own neighbour)
    rows = sorted({0, rows_per_block - 1, rows_per_block, 2 * rows_per_block - 1, 2 * rows_per_block, n_q - 1,
                   *rng.integers(0, n_q, 12).tolist()})
    q = queries[rows]
    dist_rows = oracle_both(parent, dist, _grid_pairs(q, cands, 0, len(q) * len(cands)))[0].reshape(len(q), len(cands))
    want_idx, want_d = _knn_want(dist_rows, q, cands, k, True)
    assert np.array_equal(idx[rows], want_idx), (rows, idx[rows], want_idx)
    assert_bits_equal(d[rows], want_d, "rows at the block edges")
    # without skip_self every leaf query finds a candidate at distance 0 (itself, or one listed earlier at distance 0)
    idx0, d0 = dev.knn_host(queries, cands, 2, skip_self=False)
    assert (d0[:, 0] == 0).all()
    want_idx0, want_d0 = _knn_want(dist_rows, q, cands, 2, False)
    assert np.array_equal(idx0[rows], want_idx0)
    assert_bits_equal(d0[rows], want_d0, "rows at the block edges, skip_self=0")
    dev.close()


# ---- E. graph matrices and the unpack kernel -----------------------------------------------------------------------

def _graph_want(n, u, v, w):
    A = np.zeros((n, n))
    A[u, v] = w
    A[v, u] = w
    return A, np.diag(A.sum(axis=0)) - A


def _random_simple_graph(n, n_edges, rng):
    """n_edges distinct undirected edges without self-loops, random orientation, weights of either sign.  (Duplicate edges
    are last-writer-wins on the host and a race between lanes on the device: not a defined input, not tested.)"""
    code = rng.choice(n * (n - 1) // 2, n_edges, replace=False)
    i, j = np.tril_indices(n, -1)
    u, v = i[code].astype(np.int32), j[code].astype(np.int32)
    flip = rng.random(n_edges) < 0.5
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    w = rng.normal(0.0, 2.0, n_edges)
    return u, v, w


def test_e_graph_matrices_against_numpy():
    """st_graph_matrices_host against A[u,v] = A[v,u] = w and diag(A.sum(axis=0)) - A in float64, bit for bit: one node
    without edges, 65 nodes, 4200 nodes (k_graph_laplacian's grid-stride loop runs twice) and more than 1,048,576 edges
    (k_graph_scatter's does); negative weights and a self-loop; either output alone and both."""
    rng = np.random.default_rng(33)
    empty = np.zeros(0, np.int32)
    A, L = _capi.graph_matrices(1, empty, empty, np.zeros(0))
    assert A.shape == L.shape == (1, 1) and A[0, 0] == 0 and L[0, 0] == 0
    for n, n_edges in ((65, 300), (4200, 20_000), (4200, GRAPH_SCATTER_SPAN + 4097)):
        assert n_edges <= n * (n - 1) // 2
        u, v, w = _random_simple_graph(n, n_edges, rng)
        u, v, w = np.append(u, 7).astype(np.int32), np.append(v, 7).astype(np.int32), np.append(w, -3.25)      # a self-loop
        assert (w < 0).sum() > n_edges // 3
        if n == 4200:
            assert n * n > GRAPH_LAPLACIAN_SPAN
        want_a, want_l = _graph_want(n, u, v, w)
        for adj, lap in ((True, True), (True, False), (False, True)):
            A, L = _capi.graph_matrices(n, u, v, w, want_adjacency=adj, want_laplacian=lap)
            assert (A is None) == (not adj) and (L is None) == (not lap)
            if adj:
                assert np.array_equal(A.view(np.int64), want_a.view(np.int64)), (n, n_edges, "adjacency")
            if lap:
                assert np.array_equal(L.view(np.int64), want_l.view(np.int64)), (n, n_edges, "laplacian")
        bad = u.copy()
        bad[len(bad) // 2] = n
        with pytest.raises(ValueError):
            _capi.graph_matrices(n, bad, v, w)
        with pytest.raises(ValueError):
            _capi.graph_matrices(n, u, np.where(np.arange(len(v)) == 3, -1, v), w)


def test_e_unpack_mrca24_at_every_alignment():
    """st_unpack_mrca24_device: 1, 2, 3 and 5 ids starting at each of the four byte alignments, poison before and after the
    packed bytes, 0xFFFFFF -> -1 at the first and the last position."""
    import torch
    dev = _capi.DeviceTree(*synth.balanced_tree(4))
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 5):
        for off in range(4):
            for minus_one in ((), (0,), (n - 1,), (0, n - 1)):
                ids = rng.integers(0, 0xFFFFFF, n).astype(np.int64)
                ids[0] = 0xFFFFFE if n > 1 else ids[0]
                want = ids.copy()
                for p in minus_one:
                    ids[p], want[p] = 0xFFFFFF, -1
                raw = np.full(64, 0xAB, dtype=np.uint8)
                for i, x in enumerate(ids):
                    raw[off + 3 * i: off + 3 * i + 3] = [x & 0xFF, (x >> 8) & 0xFF, (x >> 16) & 0xFF]
                packed = torch.from_numpy(raw).cuda()
                assert packed.data_ptr() % 4 == 0
                out = torch.full((n + 4,), -7, dtype=torch.int32, device="cuda")
                dev.unpack_mrca24_device(packed.data_ptr() + off, n, out.data_ptr())
                got = out.cpu().numpy()
                assert got[:n].tolist() == want.tolist() and (got[n:] == -7).all(), (n, off, minus_one, got)
    dev.close()
