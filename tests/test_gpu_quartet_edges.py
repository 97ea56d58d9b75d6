"""The quartet comparison at its launch, chunk and polytomy edges (kernels_quartets.h, host_quartets.h), against the
references of tests/quartet_reference.py, which share nothing with the library.  Every expectation is exact equality of
integers.

A  the generator past one launch (1024 x 256 lanes) and one chunk (2^22 quartets): all quartets of 103 leaves, windows on
   every kind of block edge of the unranking at 65536 leaves, draws at the ends of the leaf range
B  batches whose every row votes for a cell the test chose, on the lane, wave, block, grid and chunk seams of the count
C  trees of any arity and numbering -- the general records, class 3 from the tree's own shape -- against the four-point
   rule; star trees; what the Newick ingest makes of a polytomy
D  one cell past 2^32: all 5,346,164,850 quartets of a 600-leaf caterpillar against a star
"""
import math
import time

import numpy as np
import pytest

import quartet_reference as qr
from oracle.oracle import OracleTree
from suchtree_amd import SuchTree, _capi, synth
from suchtree_amd.compare import quartet_positions

pytestmark = pytest.mark.gpu

GRID = 1024 * 256                    # kernels_quartets.h: kQuartetBlocks x kQuartetThreads, the lanes of one launch
CHUNK = 1 << 22                      # host_quartets.h: kQuartetChunk
M_ALL = 65536                        # quartet_plan.h: kQuartetMaxLeavesAll
M64 = (1 << 64) - 1


# ---- A. the generator -----------------------------------------------------------------------------------------------
def test_all_quartets_of_103_leaves_two_chunks_and_seventeen_grid_trips():
    want = qr.colex_quartets(103)
    assert len(want) == CHUNK + 226_971 and -(-len(want) // GRID) == 17
    got = quartet_positions(103, device=0)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, "%d rows differ, first %d: got %s want %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


def outer_edges():
    """p whose block edge C(p,4) a window straddles: the smallest, the largest, powers of two and their neighbours, a
    seeded spread."""
    ps = {4, 5, 6, M_ALL - 1, M_ALL}
    for e in range(3, 16):
        ps |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    ps |= set(np.random.default_rng(65).integers(7, M_ALL, 8).tolist())
    return sorted(ps)


def inner_edges():
    """k = C(p3,4) + C(p2,3) and k = C(p3,4) + C(p2,3) + C(p1,2): where p2, and where p1, steps."""
    ks = []
    for p3 in (5, 6, 100, 4097, 40_000, M_ALL - 1):
        for p2 in sorted({2, 3, p3 // 2, p3 - 2, p3 - 1}):
            ks.append(math.comb(p3, 4) + math.comb(p2, 3))
            for p1 in sorted({1, p2 // 2, p2 - 1} - {0}):
                ks.append(math.comb(p3, 4) + math.comb(p2, 3) + math.comb(p1, 2))
    return sorted(set(ks))


def check_window(centre):
    """The 128 quartets around index ``centre`` (those that exist) from the device, against unrank_exact."""
    lo, hi = max(0, centre - 64), min(math.comb(M_ALL, 4), centre + 64)
    got = quartet_positions(M_ALL, begin=lo, count=hi - lo, device=0)
    want = [qr.unrank_exact(k) for k in range(lo, hi)]
    assert got.tolist() == want, "window [%d, %d)" % (lo, hi)
    return hi - lo


def test_unranking_windows_on_the_block_edges_of_65536_leaves():
    ps = outer_edges()
    assert len(ps) >= 40 and {4, 5, 6, 4096, 65535} <= set(ps)
    sizes = {p: check_window(math.comb(p, 4)) for p in ps}
    assert sizes[4] == 65 and sizes[5] == 69 and sizes[6] == 79 and sizes[M_ALL] == 64 and sizes[M_ALL - 1] == 128
    # the edge itself, spelled out: the last quartet below p and the first with p
    for p in (4, 1000, M_ALL - 1):
        got = quartet_positions(M_ALL, begin=math.comb(p, 4) - 1, count=2, device=0)
        assert got.tolist() == [[p - 4, p - 3, p - 2, p - 1], [0, 1, 2, p]]


def test_unranking_windows_on_the_inner_edges_of_65536_leaves():
    ks = inner_edges()
    assert len(ks) >= 40
    for k in ks:
        check_window(k)


N_DRAW = CHUNK + GRID + 65           # a second chunk that makes a second grid trip and ends in a partial wave
DRAW_AT = [0, 63, 64, 255, 256, GRID - 1, GRID, CHUNK - 1, CHUNK, N_DRAW - 1]


@pytest.mark.parametrize("seed", [0, M64])
@pytest.mark.parametrize("m", [2 ** 31 - 1, 5, 4])
def test_draws_past_one_chunk_equal_the_host_and_python(m, seed):
    at = np.concatenate([DRAW_AT, np.random.default_rng(m % 1000).integers(0, N_DRAW, 2000)])
    for begin in (0, CHUNK - 3):      # (the second request's chunks begin in mid-range)
        want = quartet_positions(m, samples=begin + N_DRAW, seed=seed, begin=begin)
        got = quartet_positions(m, samples=begin + N_DRAW, seed=seed, begin=begin, device=0)
        assert got.shape == (N_DRAW, 4)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "begin %d: %d rows differ, first %d" % (begin, len(bad), bad[0])
        assert got[at].tolist() == [qr.py_draw(seed, begin + int(i), m) for i in at], begin


# ---- B. painted batches ---------------------------------------------------------------------------------------------
QUAD = "((a:1,b:1):1,(c:1,d:1):1);"
PAINT_N = [1, 63, 64, 65, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * GRID + 65]


class Painter:
    """One four-leaf tree on both sides; rows[c] is a row of class c: (a,b,c,d), (a,c,b,d), (a,c,d,b), (a,a,a,a)."""

    def __init__(self, strategy="auto"):
        self.T = SuchTree(QUAD, strategy=strategy)
        a, b, c, d = (self.T.leaves[k] for k in "abcd")
        self.rows = np.array([[a, b, c, d], [a, c, b, d], [a, c, d, b], [a, a, a, a]], dtype=np.int64)
        self.dev = self.T._device_tree()

    def table(self, cells, chunk_quartets=0):
        cells = np.asarray(cells, dtype=np.int64)
        return self.dev.compare_quartets_host(self.dev, self.rows[cells // 4], self.rows[cells % 4], chunk_quartets=chunk_quartets)


def painted(cells):
    return np.bincount(np.asarray(cells, dtype=np.int64), minlength=16).reshape(4, 4)


def paints(n):
    i = np.arange(n, dtype=np.int64)
    return {"i mod 16": i % 16,
            "wave-uniform": (i // 64) % 16,
            "cell 0 but lane 63": np.where(i % 64 == 63, 9, 0),
            "cell 5 but the last row": np.where(i == n - 1, 14, 5)}


@pytest.fixture(scope="module")
def painter():
    return Painter()


def test_the_four_painted_rows_have_the_classes_the_paint_assumes(painter):
    for c in range(4):
        want = np.zeros((4, 4), dtype=np.int64)
        want[c, 0] = 1
        assert np.array_equal(painter.table([4 * c]), want), c
        assert np.array_equal(painter.table([c]), want.T), c


@pytest.mark.parametrize("cell", range(16))
def test_every_cell_alone_over_257_rows(painter, cell):
    want = np.zeros(16, dtype=np.int64)
    want[cell] = 257
    assert np.array_equal(painter.table(np.full(257, cell)), want.reshape(4, 4))


@pytest.mark.parametrize("n", PAINT_N)
def test_painted_batches_on_the_wave_block_and_grid_seams(painter, n):
    for name, cells in paints(n).items():
        got = painter.table(cells)
        assert np.array_equal(got, painted(cells)), "%s: got %s" % (name, got.tolist())


@pytest.mark.parametrize("chunk", [0, 64, 257, GRID + 1])
def test_painted_batches_in_chunks(painter, chunk):
    for name, cells in paints(PAINT_N[-1]).items():
        got = painter.table(cells, chunk_quartets=chunk)
        assert np.array_equal(got, painted(cells)), "%s: got %s" % (name, got.tolist())


def test_painted_batches_on_walk_strategy_handles():
    p = Painter(strategy="walk")
    assert p.T.device_info()["strategy"] == "walk"
    for n in (257, PAINT_N[-1]):
        for name, cells in paints(n).items():
            got = p.table(cells)
            assert np.array_equal(got, painted(cells)), "%d %s: got %s" % (n, name, got.tolist())


# ---- C. polytomies and general-arity trees --------------------------------------------------------------------------
GENERAL_LEAVES = 300
GENERAL_SEED = 11                    # chosen on the CPU: the reference's table of the sample below has its rows filled
N_FIRST = 30                         # all C(30, 4) = 27,405 quartets of the first 30 listed leaves
N_SAMPLE = 100_003                   # 6 n is past the canopy threshold
N_SMALL = 500                        # 6 n below it
SAMPLE_SEED = 0xBEEF


class General:
    """X: a tree of arities 2 to 5 in a shuffled numbering; Y: a binary in-order tree over as many leaves, its ids
    aligned through a permutation.  The classes of both are the four-point rule's, over positions from Python."""

    def __init__(self):
        self.x = qr.random_general_tree(GENERAL_LEAVES, GENERAL_SEED)
        yp, yd = synth.random_binary_tree(GENERAL_LEAVES, seed=GENERAL_SEED)
        self.y = (yp, yd, np.random.default_rng(GENERAL_SEED).permutation(np.arange(GENERAL_LEAVES, dtype=np.int64) * 2))
        first = qr.colex_quartets(N_FIRST)
        sample = np.array([qr.py_draw(SAMPLE_SEED, k, GENERAL_LEAVES) for k in range(N_SAMPLE)], dtype=np.int64)
        self.classes = {}
        for side, (parent, _, ids) in (("x", self.x), ("y", self.y)):
            D = qr.mrca_matrices(parent, ids)[0]
            self.classes[side] = {"first": qr.leaf_classes(parent, ids[:N_FIRST], first, D=D[:N_FIRST, :N_FIRST]),
                                  "sample": qr.leaf_classes(parent, ids, sample, D=D)}
        self.handles = {}

    def handle(self, side, strategy):
        if (side, strategy) not in self.handles:
            parent, dist, _ = getattr(self, side)
            self.handles[side, strategy] = _capi.DeviceTree(parent, dist, strategy=strategy)
        return self.handles[side, strategy]


@pytest.fixture(scope="module")
def general():
    return General()


def test_the_general_tree_case_is_not_vacuous(general):
    want = qr.table_of(general.classes["x"]["sample"], general.classes["y"]["sample"])
    assert want.sum() == N_SAMPLE and (want.sum(axis=1) >= 1000).all(), want.tolist()
    assert want[:, 3].sum() == 0                      # Y is binary
    first = qr.table_of(general.classes["x"]["first"], general.classes["y"]["first"])
    assert first[3].sum() >= 1000 and (first.sum(axis=1) > 0).all(), first.tolist()
    parent, _, ids = general.x
    assert np.bincount(parent[parent >= 0]).max() == 5 and (ids % 2).any()


@pytest.mark.parametrize("strategy", ["auto", "walk"])
@pytest.mark.parametrize("sides", ["xy", "yx", "xx"])
def test_general_trees_equal_the_four_point_rule(general, sides, strategy):
    a, b = sides
    da, db = general.handle(a, strategy), general.handle(b, strategy)
    if strategy == "walk":
        assert da.info()["strategy"] == "walk"
    ids_a, ids_b = getattr(general, a)[2], getattr(general, b)[2]
    ca, cb = general.classes[a], general.classes[b]
    got = da.compare_quartets_leaves_host(db, ids_a[:N_FIRST], ids_b[:N_FIRST])
    assert np.array_equal(got, qr.table_of(ca["first"], cb["first"])), got.tolist()
    for n in (N_SAMPLE, N_SMALL):
        got = da.compare_quartets_leaves_host(db, ids_a, ids_b, mode="sample", seed=SAMPLE_SEED, k_count=n)
        assert np.array_equal(got, qr.table_of(ca["sample"][:n], cb["sample"][:n])), (n, got.tolist())


def test_star_trees():
    sp, sd, s_ids = qr.star(64)
    S = _capi.DeviceTree(sp, sd)
    n = math.comb(64, 4)
    want = np.zeros((4, 4), dtype=np.int64)
    want[3, 3] = n
    assert np.array_equal(S.compare_quartets_leaves_host(S, s_ids, s_ids), want)
    # against a perfect tree whose leaves are listed in a shuffled order: row 3 holds the perfect tree's classes
    perm = np.random.default_rng(64).permutation(64)
    counts = np.bincount(qr.perfect_classes(6, perm[qr.colex_quartets(64)]), minlength=4)
    assert counts.sum() == n and counts[3] == 0 and counts[:3].min() > 1000
    want = np.zeros((4, 4), dtype=np.int64)
    want[3] = counts
    pp, pd, p_ids = qr.perfect_tree(6)                       # heap numbering: the general records
    assert np.array_equal(S.compare_quartets_leaves_host(_capi.DeviceTree(pp, pd), s_ids, p_ids[perm]), want)
    bp, bd = synth.balanced_tree(6)                          # in-order numbering: the parity layout and the rank table
    B = _capi.DeviceTree(bp, bd)
    assert np.array_equal(S.compare_quartets_leaves_host(B, s_ids, 2 * perm), want)
    assert np.array_equal(B.compare_quartets_leaves_host(S, 2 * perm, s_ids), want.T)


def test_all_quartets_of_103_shuffled_leaves_cross_the_default_chunk_on_the_compare_path():
    """Two chunks and seventeen grid trips again, this time through the id rows and the count, with classes that depend on
    which quartet a lane was given: 103 leaves of a perfect tree of 128 in two shuffled orders (closed form)."""
    pos = qr.colex_quartets(103)
    rng = np.random.default_rng(103)
    perm_x, perm_y = rng.permutation(128)[:103], rng.permutation(128)[:103]
    cx, cy = qr.perfect_classes(7, perm_x[pos]), qr.perfect_classes(7, perm_y[pos])
    want = qr.table_of(cx, cy)
    assert want.sum() == CHUNK + 226_971 and want[:3, :3].min() > 100_000 and want[3].sum() == 0
    bp, bd = synth.balanced_tree(7)                          # in-order numbering: leaf i is node 2 i
    pp, pd, p_ids = qr.perfect_tree(7)                       # heap numbering
    X, Y = _capi.DeviceTree(bp, bd), _capi.DeviceTree(pp, pd)
    assert np.array_equal(X.compare_quartets_leaves_host(Y, 2 * perm_x, p_ids[perm_y]), want)
    assert np.array_equal(Y.compare_quartets_leaves_host(X, p_ids[perm_y], 2 * perm_x, chunk_quartets=GRID + 1), want.T)
    # a range that begins three quartets before the chunk's end
    k = CHUNK - 3
    got = X.compare_quartets_leaves_host(Y, 2 * perm_x, p_ids[perm_y], k_begin=k)
    assert np.array_equal(got, qr.table_of(cx[k:], cy[k:]))


def test_newick_polytomies_are_resolved_at_ingest_not_counted_as_unresolved():
    """the ingest resolves a polytomy with epsilon edges, as the reference does; the comparison sees a
    binary tree."""
    P = SuchTree("(a:1,b:1,c:1,d:1,e:1);")
    Q = SuchTree("((a:1,d:1):1,((b:1,e:1):1,c:1):1);")
    names = ["a", "b", "c", "d", "e"]
    pos = qr.colex_quartets(5)

    def classes(T):
        ids = np.array([T.leaves[k] for k in names], dtype=np.int64)
        q = ids[pos]
        out = OracleTree(T._flat.parent, T._flat.distance).quartets(np.ascontiguousarray(q))
        at = np.argmax(out == q[:, :1], axis=1)
        sister = out[np.arange(len(q)), at ^ 1]
        return np.argmax(q[:, 1:] == sister[:, None], axis=1)
    for A, B in ((P, P), (P, Q), (Q, P)):
        r = A.compare_quartets(B, leaves=names)
        assert r.n == 5 and r.unresolved == 0
        assert np.array_equal(r.table, qr.table_of(classes(A), classes(B)))


# ---- D. one cell past 2^32 ------------------------------------------------------------------------------------------
def test_one_cell_past_two_to_the_32():
    """All quartets of 600 leaves, a caterpillar (leaves in depth order: class 0) against a star (class 3): 1275 chunks,
    one cell of 5,346,164,850 > 2^32 behind 32-bit wave and LDS counters.  0.53 s on the MI355X (LAB_NOTES.md)."""
    for m in (40, 600):
        cp, cd = synth.caterpillar_tree(m)
        sp, sd, s_ids = qr.star(m)
        c_ids = np.arange(m, dtype=np.int64) * 2             # depth order: leaves 0 and 2 are the deepest
        C, S = _capi.DeviceTree(cp, cd), _capi.DeviceTree(sp, sd)
        if m == 40:
            pos = qr.colex_quartets(m)
            want = qr.table_of(qr.leaf_classes(cp, c_ids, pos), qr.leaf_classes(sp, s_ids, pos))
        else:
            want = qr.table_of(qr.caterpillar_classes(np.arange(4).reshape(1, 4)), qr.star_classes(np.zeros((1, 4)))) * math.comb(m, 4)
        assert want[0, 3] == math.comb(m, 4) == want.sum()
        t0 = time.perf_counter()
        got = C.compare_quartets_leaves_host(S, c_ids, s_ids)
        print("all quartets of %d leaves, caterpillar against star: %.3f s" % (m, time.perf_counter() - t0))
        assert got.dtype == np.int64 and np.array_equal(got, want), got.tolist()
    assert got[0, 3] == 5_346_164_850 > 1 << 32 and got.sum() == 5_346_164_850
