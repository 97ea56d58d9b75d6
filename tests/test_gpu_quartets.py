"""Two trees compared by quartet topology on the GPU (SuchTree.compare_quartets, C ABI st_compare_quartets_*_host,
st_quartet_positions): the device generator against its host restatement, known answers, and the literal 4 x 4 table
against the oracle's quartet topologies of both trees over the host-restated positions."""
import math

import numpy as np
import pytest

from conftest import golden_path
from oracle.oracle import OracleTree
from suchtree_amd import InvalidNodeError, SuchTree, _capi, synth
from suchtree_amd.compare import QuartetComparison, quartet_positions

pytestmark = pytest.mark.gpu

N_ALL_LEAVES = 40            # C(40, 4) = 91,390 quartets
N_SAMPLE = 100_003           # 6 n is past kCanopyMinPairs: the rank-table / canopy kernels
N_SMALL = 500                # 6 n below it: the small-batch path
SEED = 0xC0FFEE


def oracle_classes(O, quartets):
    """Class of each row (distinct ids) from OracleTree.quartets: which input column ends up beside column 0."""
    q = np.ascontiguousarray(quartets, dtype=np.int64)
    out = O.quartets(q)
    at = np.argmax(out == q[:, :1], axis=1)                 # where column 0 went
    partner = out[np.arange(len(q)), at ^ 1]                # its sister
    cls = np.argmax(q[:, 1:] == partner[:, None], axis=1)   # input column 1, 2 or 3 -> class 0, 1, 2
    assert (out[np.arange(len(q)), at] == q[:, 0]).all() and (q[np.arange(len(q)), cls + 1] == partner).all()
    return cls


def table_of(cx, cy):
    t = np.zeros((4, 4), dtype=np.int64)
    np.add.at(t, (cx, cy), 1)
    return t


def pick_classes(m6):
    """The pick rule over (n, 6) MRCA ids, in numpy: class 3 where no id is unique."""
    counts = (m6[:, :, None] == m6[:, None, :]).sum(axis=2)
    unique = counts == 1
    pick = np.where(unique.any(axis=1), np.argmax(unique, axis=1), 6)
    return np.where(pick == 6, 3, np.where(pick < 3, pick, 5 - pick))


class Case:
    """Two trees over aligned id lists, with the oracle's classes of all quartets of the first 40 ids and of a sample."""

    def __init__(self, x, y, ids_x, ids_y, strategy="auto"):
        (px, dx), (py, dy) = x, y
        self.ids_x, self.ids_y = np.ascontiguousarray(ids_x, dtype=np.int64), np.ascontiguousarray(ids_y, dtype=np.int64)
        self.m = len(self.ids_x)
        self.Ox, self.Oy = OracleTree(px, dx), OracleTree(py, dy)
        self.Tx, self.Ty = SuchTree((px, dx), strategy=strategy), SuchTree((py, dy), strategy=strategy)
        self.walk = {}
        pos = quartet_positions(N_ALL_LEAVES)
        self.all_x = oracle_classes(self.Ox, self.ids_x[:N_ALL_LEAVES][pos])
        self.all_y = oracle_classes(self.Oy, self.ids_y[:N_ALL_LEAVES][pos])
        pos = quartet_positions(self.m, samples=N_SAMPLE, seed=SEED)
        self.sample_x = oracle_classes(self.Ox, self.ids_x[pos])
        self.sample_y = oracle_classes(self.Oy, self.ids_y[pos])

    def walk_trees(self):
        if not self.walk:
            self.walk = {"x": SuchTree((self.Tx._flat.parent, self.Tx._flat.distance), strategy="walk"),
                         "y": SuchTree((self.Ty._flat.parent, self.Ty._flat.distance), strategy="walk")}
        return self.walk["x"], self.walk["y"]


@pytest.fixture(scope="module")
def cases(ml_arrays, nj_arrays):
    out = {}
    even = lambda n: np.arange(n, dtype=np.int64) * 2      # noqa: E731  (leaves of the synthetic trees: the even ids)
    out["random"] = Case(synth.random_binary_tree(3000, seed=1), synth.random_binary_tree(3000, seed=2), even(3000), even(3000))
    bal = synth.balanced_tree(10)
    out["balanced"] = Case(bal, bal, even(1024), np.random.default_rng(3).permutation(even(1024)))
    out["caterpillar"] = Case(synth.caterpillar_tree(600), synth.random_binary_tree(600), even(600),
                              np.random.default_rng(4).permutation(even(600)))
    p1, d1, leaves1 = ml_arrays
    p2, d2, _ = nj_arrays
    nj_of = np.load(golden_path("ml_nj_leaf_map.npz"))["nj_id_of_ml_leaf"].astype(np.int64)
    sel = np.random.default_rng(21).choice(len(leaves1), 3000, replace=False)
    out["ml_nj"] = Case((p1, d1), (p2, d2), leaves1[sel], nj_of[sel])
    return out


CASES = ("random", "balanced", "caterpillar", "ml_nj")


# ---- the generator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 5, 37])
def test_device_unranking_equals_the_host_restatement(m):
    want = quartet_positions(m)
    got = quartet_positions(m, device=0)
    assert got.shape == (math.comb(m, 4), 4) and got.dtype == np.int32 and np.array_equal(got, want)


def test_device_unranking_at_the_end_of_the_largest_leaf_set():
    total = math.comb(65536, 4)
    want = quartet_positions(65536, begin=total - 10_000)
    got = quartet_positions(65536, begin=total - 10_000, device=0)
    assert len(got) == 10_000 and np.array_equal(got, want)
    assert got[-1].tolist() == [65532, 65533, 65534, 65535]


@pytest.mark.parametrize("m, seed", [(2 ** 31 - 1, 0), (2 ** 31 - 1, 2 ** 64 - 1), (4, 1), (1000, SEED)])
def test_device_draw_equals_the_host_restatement(m, seed):
    want = quartet_positions(m, samples=N_SAMPLE, seed=seed)
    got = quartet_positions(m, samples=N_SAMPLE, seed=seed, device=0)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() < m and (np.sort(got, axis=1)[:, 1:] > np.sort(got, axis=1)[:, :-1]).all()
    # the prefix property, through a k_begin on the device
    tail = quartet_positions(m, samples=N_SAMPLE, seed=seed, begin=N_SAMPLE - 1000, device=0)
    assert np.array_equal(tail, want[-1000:])


# ---- known answers --------------------------------------------------------------------------------------------------
def test_two_resolutions_of_one_quartet():
    X, Y = SuchTree("((a:1,b:1):1,(c:1,d:1):1);"), SuchTree("((a:1,c:1):1,(b:1,d:1):1);")
    c = X.compare_quartets(Y, leaves=["a", "b", "c", "d"])
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 1] = 1
    assert c.n == 1 and np.array_equal(c.table, want) and c.agree == 0 and c.distance == 1.0 and c.mode == "all" and c.n_leaves == 4
    assert np.array_equal(X.compare_quartets(Y).table, want)                 # the shared leaves, in X's leaf order: a b c d
    g = X.compare_quartets(Y, quartets=[("a", "c", "b", "d")])                # rows (a,c,b,d): X joins the 1st and 3rd, Y the 1st and 2nd
    assert g.mode == "given" and g.table[1, 0] == 1 and g.n == 1
    # caterpillars whose only unique MRCA is that of the cherry without a: picks 5, 4 and 3
    names = ["a", "b", "c", "d"]
    P5, P4, P3 = SuchTree("(((c:1,d:1):1,b:1):1,a:1);"), SuchTree("(((b:1,d:1):1,c:1):1,a:1);"), SuchTree("(((b:1,c:1):1,d:1):1,a:1);")
    for A, B, cell in ((P5, P4, (0, 1)), (P4, P3, (1, 2)), (P3, P5, (2, 0)), (P5, X, (0, 0)), (P4, Y, (1, 1))):
        t = A.compare_quartets(B, leaves=names).table
        assert t.sum() == 1 and t[cell] == 1, cell


def test_two_hand_checked_trees_of_five_leaves():
    names = ["a", "b", "c", "d", "e"]
    T1 = SuchTree("(((a:1,b:1):1,c:1):1,(d:1,e:1):1);")
    T2 = SuchTree("(((a:1,c:1):1,b:1):1,(d:1,e:1):1);")
    T3 = SuchTree("((a:1,d:1):1,((b:1,e:1):1,c:1):1);")
    # quartets in colexicographic order: abcd abce abde acde bcde
    # T1: ab|cd ab|ce ab|de ac|de bc|de -> 0 0 0 0 0;  T2: ac|bd ac|be ab|de ac|de bc|de -> 1 1 0 0 0
    # T3: ad|bc ac|be ad|be ad|ce be|cd -> 2 1 1 1 2
    c12 = T1.compare_quartets(T2, leaves=names)
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 0], want[0, 1] = 3, 2
    assert np.array_equal(c12.table, want) and c12.agree == 3 and abs(c12.distance - 0.4) < 1e-15 and c12.stderr == 0.0
    c13 = T1.compare_quartets(T3, leaves=names)
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 1], want[0, 2] = 3, 2
    assert np.array_equal(c13.table, want) and c13.distance == 1.0
    c23 = T2.compare_quartets(T3, leaves=names)
    want = np.zeros((4, 4), dtype=np.int64)
    want[1, 2], want[1, 1], want[0, 1], want[0, 2] = 1, 1, 2, 1
    assert np.array_equal(c23.table, want) and c23.agree == 1 and c23.unresolved == 0


def test_a_tree_against_itself_over_all_quartets_of_37_leaves(cases):
    c = cases["random"]
    ids = c.ids_x[:37]
    r = c.Tx.compare_quartets(c.Tx, leaves=(ids, ids))
    assert r.n == math.comb(37, 4) == 66045 and r.table.sum() == r.n
    assert np.array_equal(r.table, np.diag(np.diag(r.table))) and r.distance == 0.0 and r.similarity == 1.0
    assert r.table[3, :].sum() == 0 and r.table[:, 3].sum() == 0 and r.unresolved == 0


# ---- the oracle's table, literally ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_all_quartets_of_40_leaves_equal_the_oracle(cases, name):
    c = cases[name]
    r = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x[:N_ALL_LEAVES], c.ids_y[:N_ALL_LEAVES]))
    assert r.n == 91_390 and r.mode == "all" and r.seed is None and r.n_leaves == N_ALL_LEAVES
    assert np.array_equal(r.table, table_of(c.all_x, c.all_y))


@pytest.mark.parametrize("name", CASES)
def test_samples_equal_the_oracle(cases, name):
    c = cases[name]
    r = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=N_SAMPLE, seed=SEED)
    assert r.n == N_SAMPLE and r.mode == "sample" and r.seed == SEED and r.n_leaves == c.m
    want = table_of(c.sample_x, c.sample_y)
    assert np.array_equal(r.table, want)
    assert r.agree == int((c.sample_x == c.sample_y).sum()) and r.unresolved == 0
    assert abs(r.stderr - math.sqrt(r.similarity * (1 - r.similarity) / r.n)) < 1e-15
    # the small-batch path: the first 500 quartets of the same sample
    s = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=N_SMALL, seed=SEED)
    assert np.array_equal(s.table, table_of(c.sample_x[:N_SMALL], c.sample_y[:N_SMALL]))


@pytest.mark.parametrize("name", CASES)
def test_walk_strategy_trees_equal_the_oracle(cases, name):
    c = cases[name]
    Wx, Wy = c.walk_trees()
    assert Wx.device_info()["strategy"] == "walk"
    r = Wx.compare_quartets(Wy, leaves=(c.ids_x, c.ids_y), samples=N_SAMPLE, seed=SEED)
    assert np.array_equal(r.table, table_of(c.sample_x, c.sample_y))
    a = Wx.compare_quartets(Wy, leaves=(c.ids_x[:N_ALL_LEAVES], c.ids_y[:N_ALL_LEAVES]))
    assert np.array_equal(a.table, table_of(c.all_x, c.all_y))


@pytest.mark.parametrize("name", CASES)
def test_chunks_and_ranges_do_not_change_the_table(cases, name):
    c = cases[name]
    dx, dy = c.Tx._device_tree(), c.Ty._device_tree()
    want = table_of(c.sample_x, c.sample_y)
    for chunk in (0, 1000, 65536):
        got = dx.compare_quartets_leaves_host(dy, c.ids_x, c.ids_y, mode="sample", seed=SEED, k_count=N_SAMPLE, chunk_quartets=chunk)
        assert np.array_equal(got, want), chunk
    ids_x, ids_y = c.ids_x[:N_ALL_LEAVES], c.ids_y[:N_ALL_LEAVES]
    want_all = table_of(c.all_x, c.all_y)
    for chunk in (0, 1000, 65536):
        assert np.array_equal(dx.compare_quartets_leaves_host(dy, ids_x, ids_y, chunk_quartets=chunk), want_all), chunk
    for mode, n, kw, full, cx, cy in (("sample", N_SAMPLE, dict(ids_x=c.ids_x, ids_y=c.ids_y, seed=SEED), want, c.sample_x, c.sample_y),
                                      ("all", 91_390, dict(ids_x=ids_x, ids_y=ids_y), want_all, c.all_x, c.all_y)):
        k = 33_333
        lo = dx.compare_quartets_leaves_host(dy, mode=mode, k_begin=0, k_count=k, **kw)
        hi = dx.compare_quartets_leaves_host(dy, mode=mode, k_begin=k, k_count=n - k, **kw)
        assert np.array_equal(lo, table_of(cx[:k], cy[:k])) and np.array_equal(hi, table_of(cx[k:], cy[k:]))
        merged = QuartetComparison.merge(QuartetComparison.from_table(lo, mode=mode), QuartetComparison.from_table(hi, mode=mode))
        assert merged.n == n and np.array_equal(merged.table, full)


# ---- explicit quartets ----------------------------------------------------------------------------------------------
def test_explicit_quartets_with_repeats_and_internal_nodes(cases):
    c = cases["random"]
    rng = np.random.default_rng(12)
    n = 20_000
    qx = c.ids_x[np.stack([rng.permutation(c.m)[:4] for _ in range(n)])]      # distinct leaves
    qy = qx.copy()
    odd = np.arange(n // 2)
    qx[odd[: n // 4], rng.integers(1, 4, n // 4)] = qx[odd[: n // 4], 0]      # a repeated id
    qx[odd[n // 4:], rng.integers(0, 4, n // 2 - n // 4)] = rng.integers(0, c.m - 1, n // 2 - n // 4) * 2 + 1      # an internal node
    qy[odd] = rng.integers(0, c.Ty.size, (n // 2, 4))                         # anything at all
    combos = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    mx = np.stack([c.Ox.mrca_bulk(qx[:, list(ab)]) for ab in combos], axis=1)
    my = np.stack([c.Oy.mrca_bulk(qy[:, list(ab)]) for ab in combos], axis=1)
    want = table_of(pick_classes(mx), pick_classes(my))
    assert want[3, :].sum() > 0 and want[:, 3].sum() > 0
    r = c.Tx.compare_quartets(c.Ty, quartets=(qx, qy))
    assert r.mode == "given" and r.n == n and r.n_leaves is None and np.array_equal(r.table, want)
    assert r.unresolved == want[3, :].sum() + want[:3, 3].sum()
    dx, dy = c.Tx._device_tree(), c.Ty._device_tree()
    assert np.array_equal(dx.compare_quartets_host(dy, qx, qy, chunk_quartets=777), want)


def test_an_id_out_of_range_is_reported_and_the_next_call_works(cases):
    c = cases["random"]
    q = c.ids_x[quartet_positions(c.m, samples=100, seed=1)]
    bad = q.copy()
    bad[57, 2] = c.Tx.size + 9
    with pytest.raises(InvalidNodeError) as e:
        c.Tx.compare_quartets(c.Ty, quartets=(bad, q))
    assert str(c.Tx.size + 9) in str(e.value)
    bad[57, 2] = -4
    with pytest.raises(InvalidNodeError) as e:
        c.Tx.compare_quartets(c.Ty, quartets=(q, bad))
    assert "-4" in str(e.value)
    ids = c.ids_x.copy()
    ids[5] = c.Tx.size
    with pytest.raises(InvalidNodeError):
        c.Tx.compare_quartets(c.Ty, leaves=(ids, c.ids_y), samples=10, seed=0)
    r = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=N_SMALL, seed=SEED)
    assert np.array_equal(r.table, table_of(c.sample_x[:N_SMALL], c.sample_y[:N_SMALL]))


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_edge_cases(cases):
    c = cases["random"]
    e = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=0, seed=3)
    assert e.n == 0 and e.table.sum() == 0 and math.isnan(e.similarity)
    e = c.Tx.compare_quartets(c.Ty, quartets=(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4), dtype=np.int64)))
    assert e.n == 0 and e.table.shape == (4, 4)
    three = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x[:3], c.ids_y[:3]))
    assert three.n == 0 and three.n_leaves == 3 and three.mode == "all"
    with pytest.raises(ValueError):
        c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x[:3], c.ids_y[:3]), samples=5)
    same = c.Tx.compare_quartets(c.Tx, leaves=(c.ids_x, c.ids_x), samples=N_SAMPLE, seed=SEED)      # one tree twice: one lock, no hang
    assert np.array_equal(same.table, table_of(c.sample_x, c.sample_x)) and same.distance == 0.0
    auto = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=1000)
    assert auto.seed is not None and auto.n == 1000
    again = c.Tx.compare_quartets(c.Ty, leaves=(c.ids_x, c.ids_y), samples=1000, seed=auto.seed)
    assert np.array_equal(again.table, auto.table)
    dx, dy = c.Tx._device_tree(), c.Ty._device_tree()
    for kw in (dict(chunk_quartets=-1), dict(chunk_quartets=(2 ** 31) // 6 + 1), dict(k_begin=N_SAMPLE, k_count=2 ** 62)):
        with pytest.raises(ValueError):
            dx.compare_quartets_leaves_host(dy, c.ids_x, c.ids_y, mode="sample", seed=1, **{"k_count": 10, **kw})


def test_trees_on_different_devices_are_refused(cases):
    if _capi.device_count() < 2:
        pytest.skip("one GPU visible: the other-device case needs two")
    c = cases["balanced"]
    other = SuchTree((c.Ty._flat.parent, c.Ty._flat.distance), device=1)
    with pytest.raises(ValueError):
        c.Tx.compare_quartets(other, leaves=(c.ids_x, c.ids_y), samples=100, seed=0)
