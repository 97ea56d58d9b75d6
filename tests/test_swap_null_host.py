"""The host side of the swap null (no GPU): st_swap_null_tables(device = -1) against the chain restated in Python integers
(tests/swap_null_reference.py) value for value; the structure of a table row; the wave's batched schedule against the
serial chain; uniformity on two small margin classes; st_dispersion_matrix_swap(device = -1) against the existing
st_dispersion_matrix on the table rows' sets; the new errors in their order; the facades' defaults; the plan and the
chain under the sanitizers; the resources of the new kernels.

Uniformity.  A chain of T trials from the observation ends in a state of its margin class; over chains p = 1 .. N the
end states are independent draws, and if the chain has mixed, Pearson's chi-square of their counts against N / states
follows chi-square with states - 1 degrees of freedom.  The bound is its 1 - 1e-6 quantile: a correct sampler fails one
run in a million, and the run is seeded.  The restatement gives 3.58 (6 states, 6000 chains of 64 trials, 0.67 of the
trials accepted) and 117.6 (117 states, 20000 chains of 300 trials, 0.41 accepted); chains of 4 trials give 98671, far
above the bound: the test can fail."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import swap_null_reference as ref
from conftest import ROOT
from kernel_resources import HIPCC, resources
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

IDENTITY = ([[0], [1], [2]], 3, 12345, 7)                           # rows, columns, seed, stream
SKEWED = ([[0, 1, 2], [1, 3], [2, 4], [0]], 5, 99, 7)

CASES = {
    "identity": (3, [[0], [1], [2]]),
    "skewed": (5, [[0, 1, 2], [1, 3], [2, 4], [0]]),
    "one_row": (6, [[0, 2, 5]]),
    "rows_of_one": (7, [[3], [0], [6], [3], [1]]),
    "a_full_row": (4, [[0, 1, 2, 3], [1], [0, 3], [2]]),
    "identical_rows": (6, [[1, 4], [1, 4], [0, 5], [2, 3, 4]]),
    "an_empty_row_between": (5, [[0, 3], [], [1, 2, 4], [], [3]]),
    "word_edge": (130, [[0, 63, 64, 127, 128, 129], [1, 64], [63, 65, 128], [5]]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_tables_equal_the_python_restatement(name):
    n, rows = CASES[name]
    for iterations in (0, 1, 63, 64, 65):
        tables, offsets, accepted = _capi.swap_null_tables(rows, n, permutations=6, iterations=iterations, seed=17, stream=3)
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
        for p in range(7):
            want, a = ref.table_row(rows, p, iterations, 17, 3)
            assert tables[p].tolist() == want and accepted[p] == a, (iterations, p)
        # p_begin > 0: row p is the same as in a call from 0
        late = _capi.swap_null_tables(rows, n, permutations=2, begin=4, iterations=iterations, seed=17, stream=3)
        assert np.array_equal(late[0], tables[4:]) and np.array_equal(late[2], accepted[4:])
    if name == "a_full_row":
        assert (tables[:, :4] == np.arange(4)).all()      # the whole universe never swaps
    if name == "one_row":
        assert (accepted == 0).all() and (tables == tables[0]).all()


def test_structure_of_the_rows():
    rng = np.random.default_rng(5)
    n = 200
    rows = [np.sort(rng.choice(n, k, replace=False)) for k in rng.integers(0, 40, 60)]
    tables, offsets, accepted = _capi.swap_null_tables(rows, n, permutations=20, seed=9)      # (default iterations)
    assert np.array_equal(tables[0], np.concatenate(rows)) and accepted[0] == 0 and accepted[1:].min() > 0
    degree = np.bincount(np.concatenate(rows), minlength=n)
    for t in tables:
        assert np.array_equal(np.bincount(t, minlength=n), degree)                      # column sums
        for r in range(len(rows)):                                                       # row sums are the offsets'
            assert (np.diff(t[offsets[r]:offsets[r + 1]].astype(np.int64)) > 0).all()   # strictly increasing
    explicit = _capi.swap_null_tables(rows, n, permutations=20, iterations=max(1000, 10 * int(offsets[-1])), seed=9)
    assert np.array_equal(explicit[0], tables)      # the default is max(1000, 10 L)
    assert len({t.tobytes() for t in tables}) == 21
    fewer_links = _capi.swap_null_tables([[4]], n, permutations=3, seed=9)      # L < 2: every chain is the observation
    assert (fewer_links[0] == 4).all() and (fewer_links[2] == 0).all()


def _random_rows(rng, n, rows_of):
    return [np.sort(rng.choice(n, k, replace=False)) for k in rows_of]


@pytest.mark.parametrize("shape", ["two_rows", "hub", "many_short_rows"])
def test_batched_schedule_equals_the_serial_chain(shape):
    """st_swap_null_schedule runs the chain in the wave's batches, cut by the prefix rule that the kernel shares
    (swap_prefix, swap_plan.h)."""
    rng = np.random.default_rng(23)
    n = 150
    sizes = {"two_rows": [40, 55], "hub": [75] + [1] * 45 + [2] * 15, "many_short_rows": rng.integers(1, 6, 400).tolist()}[shape]
    rows = _random_rows(rng, n, sizes)
    links = sum(sizes)
    if shape == "hub":
        assert sizes[0] * 2 == links      # the hub row holds half the links
    for iterations in (1, 64, 65, 5000):
        tables, _, accepted = _capi.swap_null_tables(rows, n, permutations=3, iterations=iterations, seed=2, stream=1)
        for p in range(4):
            row, a, steps = _capi.swap_null_schedule(rows, n, p, iterations=iterations, seed=2, stream=1)
            assert np.array_equal(row, tables[p]) and a == accepted[p]
            if p == 0:
                assert steps == 0
                continue
            assert -(-iterations // 64) <= steps <= iterations
            if iterations == 5000:
                print("%s: %d steps for 5000 trials, mean prefix %.2f" % (shape, steps, 5000 / steps))
                if shape == "two_rows":
                    # a second lane escapes the first only if each draws one row twice and the two rows differ -- at most
                    # 2 * (1/4) * (1/4) of the batches -- and no third lane can follow: prefixes of 1, rarely 2
                    assert 5000 // 2 <= steps and steps > 5000 * 3 // 4
                if shape == "many_short_rows":
                    assert steps < 5000 // 8


def _chi_square(start, chains, iterations):
    rows, n, seed, stream = start
    tables, offsets, accepted = _capi.swap_null_tables(rows, n, permutations=chains, iterations=iterations, seed=seed, stream=stream)
    states = ref.margin_class(rows, n)
    count = dict.fromkeys(states, 0)
    for t in tables[1:]:
        count[tuple(tuple(t[offsets[r]:offsets[r + 1]].tolist()) for r in range(len(rows)))] += 1      # (outside the class: a KeyError)
    expect = chains / len(states)
    return sum((v - expect) ** 2 / expect for v in count.values()), len(states), accepted[1:].sum() / (chains * iterations)


@pytest.mark.parametrize("start,states,chains,iterations,figure", [(IDENTITY, 6, 6000, 64, 3.58), (SKEWED, 117, 20000, 300, 117.6)])
def test_chains_reach_the_uniform_distribution(start, states, chains, iterations, figure):
    x2, n_states, share = _chi_square(start, chains, iterations)
    bound = chi2.ppf(1 - 1e-6, states - 1)
    print("%d states, %d chains of %d trials: chi-square %.2f (restatement %.2f), bound %.1f, %.2f of the trials accepted"
          % (n_states, chains, iterations, x2, figure, bound, share))
    assert n_states == states
    assert x2 < bound
    assert abs(x2 - figure) < 0.01 * figure      # the library is the restatement, value for value: so is its chi-square


def test_short_chains_fail_the_uniformity_bound():
    x2, n_states, _ = _chi_square(SKEWED, 20000, 4)
    print("117 states, 20000 chains of 4 trials: chi-square %.0f (restatement 98671)" % x2)
    assert n_states == 117 and x2 > chi2.ppf(1 - 1e-6, 116)
    small = ref.chi_square(SKEWED[0], 5, 300, 4, 99, 7)      # the Python restatement's own counting, on fewer chains
    assert small[1] == 117


SIZES = (2, 17, 32, 33, 64, 65, 130, 1, 0)


def test_records_equal_the_taxa_labels_call_on_the_table_rows():
    rng = np.random.default_rng(31)
    n = 160
    D = (rng.random((n, n)) * 10.0 ** rng.integers(-2, 2, (n, n))).astype(np.float32)
    sets = [np.sort(rng.choice(n, k, replace=False)) for k in SIZES]      # all three size classes: <= 32, 33 .. 64, above
    rec, accepted = _capi.dispersion_matrix_swap(D, sets, 4, seed=8, iterations=4000, stream=2)
    tables, off, want_accepted = _capi.swap_null_tables(sets, n, permutations=4, iterations=4000, seed=8, stream=2)
    assert np.array_equal(accepted, want_accepted) and rec.shape == (len(sets), 5)
    for p in range(5):
        rows = [tables[p, off[r]:off[r + 1]].astype(np.int64) for r in range(len(sets))]
        want = _capi.dispersion_matrix(D, rows, 0, 0)[:, 0]
        assert rec[:, p].tobytes() == want.tobytes(), p
    assert rec[:, 1].tobytes() != rec[:, 0].tobytes()
    assert (rec[-1]["pair_sum"] == 0).all() and (rec[-2]["nearest_sum"] == 0).all()      # fewer than two positions: zero records
    for chunk in (1, 3):      # (the host form has no blocks: the argument is checked and otherwise unused)
        assert _capi.dispersion_matrix_swap(D, sets, 4, seed=8, iterations=4000, stream=2, chunk_tasks=chunk)[0].tobytes() == rec.tobytes()


def _tables_raw(n_univ, pos, off, n_sets, p_begin, n_perms, iterations, stream=0, out=True, device=-1):
    L = _capi.load()
    pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    buf = np.zeros(max(1, n_perms) * max(1, 0 if pos is None else len(pos)), dtype=np.uint16) if out else None
    rc = L.st_swap_null_tables(device, n_univ, _capi._ptr(pos), 0 if pos is None else len(pos), _capi._ptr(off), n_sets, p_begin, n_perms,
                               iterations, 1, stream, _capi._ptr(buf), None)
    return rc, _capi.last_error()


def test_errors_come_in_their_order():
    pos, off = [0, 2, 1], [0, 2, 3]
    E = _capi.ST_ERR_ARG
    assert _tables_raw(5, pos, off, 2, 0, 1, 10)[0] == 0
    # every later argument is bad as well: the first check in the order answers
    assert _tables_raw(2, pos, off, 2, -1, -1, -1, -1) == (E, "a universe of 2 positions: 3 to 16384")
    assert _tables_raw(5, pos, off, 2, -1, -1, -1, -1) == (E, "p_begin < 0")
    assert _tables_raw(5, pos, off, 2, 0, -1, -1, -1) == (E, "n_perms < 0")
    assert _tables_raw(5, pos, off, 2, 0, 1, -1, -1) == (E, "stream < 0")
    rc, msg = _tables_raw(5, [0, 0, 1], off, 2, 0, 1, -1)
    assert rc == E and "strictly increasing" in msg      # the set table before iterations
    assert _tables_raw(5, pos, off, 2, 0, 1, -1) == (E, "iterations < 0")
    assert _tables_raw(5, pos, off, 2, 0, 1, -1, device=-2) == (E, "iterations < 0")      # ... before the device
    rc, msg = _tables_raw(5, pos, off, 2, 0, 1, 10, device=-2)
    assert rc == E and "device" in msg
    assert _tables_raw(5, pos, off, 2, 0, 1, 10, out=False) == (E, "out is NULL")
    # a single chain beyond the work budget: 2^30 empty sets over 16384 columns are 2^41 bytes of bit matrix
    big = 1 << 21
    rc, msg = _tables_raw(16384, None, np.zeros(big + 1, dtype=np.int64), big, 0, 1, 10)
    assert rc == 0      # 2^21 rows x 2 KiB: 4 GiB, the budget itself
    rc, msg = _tables_raw(16384, None, np.zeros(big + 2, dtype=np.int64), big + 1, 0, 1, 10)
    assert rc == E and msg == ("the state of one chain (a table row and a bit matrix of %d x 16384 bits) is %d bytes: the work budget is %d"
                               % (big + 1, (big + 1) * 2048, 4 << 30))
    # the record call: the dispersion call's checks first, then iterations, before D and out
    L = _capi.load()
    p32, o64 = np.array(pos, dtype=np.int32), np.array(off, dtype=np.int64)

    def records(n, perms, iterations, chunk, D=None, out=None):
        rc = L.st_dispersion_matrix_swap(-1, _capi._ptr(D), n, _capi._ptr(p32), 3, _capi._ptr(o64), 2, perms, iterations, 1, 0, chunk, _capi._ptr(out), None)
        return rc, _capi.last_error()
    assert records(5, -1, -1, -1) == (E, "permutations < 0")
    assert records(5, 1, -1, -1) == (E, "chunk_tasks < 0")
    assert records(5, 1, -1, 0) == (E, "iterations < 0")
    assert records(5, 1, 10, 0) == (E, "D is NULL")
    assert records(5, 1, 10, 0, D=np.zeros((5, 5), dtype=np.float32)) == (E, "out is NULL")
    with pytest.raises(ValueError):
        _capi.swap_null_tables([[0, 1]], 4, iterations=-1)
    with pytest.raises(ValueError):
        _capi.swap_null_tables([[0, 1]], 4, begin=-1)


def test_facade_defaults_and_arguments():
    for fn in (SuchTree.dispersion, SuchLinkedTrees.partner_dispersion):
        sig = inspect.signature(fn)
        assert sig.parameters["null"].default == "taxa.labels" and sig.parameters["iterations"].default is None
    # the arguments that came before keep their places
    assert list(inspect.signature(SuchTree.dispersion).parameters)[:8] == ["self", "sets", "universe", "permutations", "seed", "stream", "keep_null",
                                                                          "chunk_tasks"]
    assert list(inspect.signature(SuchLinkedTrees.partner_dispersion).parameters)[:8] == ["self", "of", "permutations", "seed", "pool", "min_partners",
                                                                                          "max_partners", "keep_null"]
    tree = SuchTree(os.path.join(ROOT, "tests", "golden", "test.tree"))
    leaves = list(tree.leaves)[:4]
    with pytest.raises(ValueError, match="null must be"):
        tree.dispersion([leaves], null="independentswap")
    with pytest.raises(ValueError, match="iterations belongs"):
        tree.dispersion([leaves], iterations=100)
    with pytest.raises(ValueError, match="iterations"):
        tree.dispersion([leaves], null="swap", iterations=-1)
    res = compare.SetDispersion(2, 9, 1, 5)
    assert res.null == "taxa.labels" and res.iterations is None and res.swap_accepted is None
    res = compare.SetDispersion(2, 9, 1, 5, False, "swap", 1000)
    assert res.null == "swap" and res.iterations == 1000 and res.swap_accepted.shape == (10,)
    tables, offsets, accepted = compare.swap_null_tables([[0, 1], [1, 2]], 3, permutations=4, seed=1)
    assert tables.shape == (5, 4) and tables.dtype == np.uint16 and offsets.tolist() == [0, 2, 4] and accepted.shape == (5,)
    assert np.array_equal(tables, _capi.swap_null_tables([[0, 1], [1, 2]], 3, permutations=4, seed=1)[0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_swap_plan_and_chain_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_swap")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_swap.cpp"), os.path.join(csrc, "swap_plan.cpp"),
                           os.path.join(csrc, "dispersion_plan.cpp"), os.path.join(csrc, "hommola_plan.cpp"), os.path.join(csrc, "compare_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize swap ok" in out.stdout


# the first build that met the tests
VGPRS = {"k_swap_chainsILi64ELb0E": 36, "k_swap_chainsILi64ELb1E": 32, "k_swap_chainsILi1ELb0E": 20, "k_swap_tasks_packed": 32, "k_swap_tasks_wave": 30, "k_swap_tasks_group": 27}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_swap_kernels_use_no_scratch_and_spill_nothing():
    res = resources("suchtree_hip.hip")
    mine = {k: v for k, v in res.items() if "k_swap" in k}
    assert len(mine) == len(VGPRS), sorted(mine)
    for kernel, vgprs in VGPRS.items():
        (k, v), = [(k, v) for k, v in mine.items() if kernel in k]
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (k, v)
        assert v["vgpr"] == vgprs, (k, v)
