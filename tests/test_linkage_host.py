"""st_linkage_codes on the host (device = -1), _capi.linkage_codes, compare.linkage and compare.Dendrogram (CPU): the
cached chain against the naive restatement of tests/linkage_reference.py -- Python ints, a scan of every pair per step --
without ties, with ties at every step and with weights; against scipy where scipy is unambiguous; the dendrogram's
views; the argument errors; and linkage_plan.cpp as a program of its own under ASan + UBSan."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from linkage_reference import random_codes, reference_linkage, rows_of, ultrametric_codes
from suchtree_amd import _capi, compare
from suchtree_amd.newick import flat_tree_from_newick

METHODS = ("average", "single", "complete")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 33, 64, 65, 90])
@pytest.mark.parametrize("method", METHODS)
def test_every_field_of_every_row_without_ties(n, method):
    codes = random_codes(n, 10 * n)
    assert len(np.unique(codes)) == len(codes) and codes.min() >= 1 << 30
    got = _capi.linkage_codes(codes, method=method)
    assert got.dtype == _capi.LINKAGE_ROW and got.dtype.itemsize == 32 and len(got) == n - 1
    assert rows_of(got) == reference_linkage(codes, n, None, method)


@pytest.mark.parametrize("method", METHODS)
def test_ties_are_broken_by_the_stated_rule(method):
    codes = np.random.default_rng(40).integers(1, 4, size=40 * 39 // 2)
    assert rows_of(_capi.linkage_codes(codes, method=method)) == reference_linkage(codes, 40, None, method)
    rows = _capi.linkage_codes(np.full(17 * 16 // 2, 6), method=method)
    assert list(zip(rows["left"].tolist(), rows["right"].tolist())) == [(0, 1)] + [(t + 1, 16 + t) for t in range(1, 16)]
    assert (rows["num"] == 6 * rows["den"]).all() and rows["size"].tolist() == list(range(2, 18))
    assert rows_of(rows) == reference_linkage([6] * 136, 17, None, method)


def test_an_ultrametric_tree_is_recovered():
    n = 64
    codes, clades = ultrametric_codes(n, 3)
    d = compare.linkage(codes.astype(np.float64), "average", device=None)
    assert [frozenset(d.members(t)) for t in range(n - 1)] == clades      # (merged in the order of the node heights)
    assert (d.heights == 1000.0 * np.arange(1, n)).all()
    truth = compare.Dendrogram(n, "average", 0, _capi.linkage_codes(codes)).to_flat()
    mine = d.to_flat()
    ids = lambda flat: np.array([flat.leaves[str(i)] for i in range(n)])      # noqa: E731
    m = compare.match_clades(mine, ids(mine), truth, ids(truth), rooted=True, device=None)
    assert m.rf == 0 and m.exact == m.n_a == m.n_b == n - 2


def test_weights_stand_for_coincident_objects():
    w = [3, 1, 2, 1, 4, 1]
    n, big = len(w), sum(w)
    codes = random_codes(n, 6, 1, 1000)
    owner = np.repeat(np.arange(n), w)
    i, j = np.tril_indices(big, -1)
    a, b = np.maximum(owner[i], owner[j]), np.minimum(owner[i], owner[j])
    expanded = np.where(a == b, 0, codes[a * (a - 1) // 2 + np.minimum(b, a - 1)])      # (zeros between the copies of one object)
    got = _capi.linkage_codes(codes, w, "average")
    flat = _capi.linkage_codes(expanded, None, "average")
    heights = lambda rows: sorted(Fraction(int(r["num"]), int(r["den"])) for r in rows if r["num"])      # noqa: E731
    assert heights(got) == heights(flat) and len(heights(got)) == n - 1
    assert rows_of(got) == reference_linkage(codes, n, w, "average") and got["size"][-1] == big
    for method in ("single", "complete"):      # the weights enter the sizes alone
        with_w, without = _capi.linkage_codes(codes, w, method), _capi.linkage_codes(codes, None, method)
        assert all(with_w[k].tolist() == without[k].tolist() for k in ("left", "right", "num", "den")) and with_w["size"][-1] == big


def test_the_comparison_has_128_bits():
    # n = 8, weights 8192: sums reach 60 bits, cross products 89 -- a comparison in 64 bits orders these wrongly
    codes, w = np.array([2 ** 31 - 1 - k for k in range(28)]), [8192] * 8
    got = _capi.linkage_codes(codes, w, "average")
    want = reference_linkage(codes, 8, w, "average")
    assert rows_of(got) == want
    assert max(r[2] for r in want).bit_length() == 60 and max(a[2] * b[3] for a in want for b in want).bit_length() >= 89


@pytest.mark.parametrize("method", ["average", "complete"])
def test_scipy_agrees_where_it_is_unambiguous(method):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    n = 300
    codes = random_codes(n, 300)
    assert len(np.unique(codes)) == len(codes)
    sq = np.zeros((n, n))
    i, j = np.tril_indices(n, -1)
    sq[i, j] = sq[j, i] = codes
    z = hier.linkage(sq[np.triu_indices(n, 1)], method=method)
    d = compare.Dendrogram(n, method, 0, _capi.linkage_codes(codes, method=method))
    assert (z[:, 0] == d.left).all() and (z[:, 1] == d.right).all() and (z[:, 3] == d.size).all()
    assert np.abs(z[:, 2] / d.heights - 1.0).max() <= 1e-12
    members = {k: [k] for k in range(n)}
    for t, (l, r) in enumerate(z[:, :2].astype(int).tolist()):
        members[n + t] = members[l] + members[r]
        assert sorted(members[n + t]) == d.members(t)


@pytest.mark.parametrize("method", METHODS)
def test_heights_are_monotone_and_the_views_agree(method):
    n = 45
    rng = np.random.default_rng(8)
    v = rng.integers(1, 30, size=n * (n - 1) // 2) / 7.0      # ties among them
    d = compare.linkage(v, method, device=None)
    assert (d.n, d.method, len(d)) == (n, method, n - 1) and 2 ** 30 <= int(np.ldexp(v.max(), d.shift)) < 2 ** 31
    frac = [Fraction(a, b) for a, b in zip(d.num.tolist(), d.den.tolist())]
    assert all(x <= y for x, y in zip(frac, frac[1:]))
    assert d.heights.tolist() == [float(np.ldexp(a / b, -d.shift)) for a, b in zip(d.num.tolist(), d.den.tolist())]
    assert d.Z.shape == (n - 1, 4) and d.Z.dtype == np.float64 and all(getattr(d, k).dtype == np.int64 for k in ("left", "right", "size", "num", "den"))
    # the square form gives the same integers
    sq = np.zeros((n, n))
    i, j = np.tril_indices(n, -1)
    sq[i, j] = sq[j, i] = v
    again = compare.linkage(sq, method, device=None)
    assert all(getattr(again, k).tolist() == getattr(d, k).tolist() for k in ("left", "right", "size", "num", "den")) and again.shift == d.shift
    # cophenetic(): scipy's, in this library's pair order
    coph = d.cophenetic()
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    theirs = np.zeros((n, n))
    theirs[np.triu_indices(n, 1)] = hier.cophenet(d.Z)
    assert (theirs.T[i, j] == coph).all()
    # Newick: the same clades, leaves as far apart as their merge is high
    names = ["t%d" % k for k in range(n - 2)] + ["a b", "it's"]
    flat = flat_tree_from_newick(d.to_newick(names))
    assert sorted(flat.leaves) == sorted(names) and flat.size == 2 * n - 1
    parent = np.asarray(flat.parent)
    under = {}
    for name in names:
        v_ = flat.leaves[name]
        while v_ != -1:
            under.setdefault(int(v_), set()).add(names.index(name))
            v_ = int(parent[v_])
    clades = {frozenset(s) for s in under.values() if len(s) > 1}
    assert clades == {frozenset(d.members(t)) for t in range(n - 1)}
    for name in names[:5]:
        v_, total = flat.leaves[name], 0.0
        while parent[v_] != -1:
            total += float(flat.distance[v_])
            v_ = int(parent[v_])
        assert total == pytest.approx(d.heights[-1] / 2, rel=1e-5)      # (ultrametric: every leaf as deep as the root is high; float32 branches)
    assert d.to_flat().num_leaves == n and sorted(d.to_flat().leaves) == sorted(str(k) for k in range(n))


def test_argument_errors():
    ok = random_codes(5, 1, 1, 100)
    with pytest.raises(ValueError, match="n = 1 objects: 2 to 16384"):
        _capi.linkage_codes(np.zeros(0, dtype=np.int32))
    with pytest.raises(ValueError, match=r"codes\[3\] = -2 is negative"):
        _capi.linkage_codes([1, 2, 3, -2, 5, 6])
    with pytest.raises(ValueError, match=r"weights\[1\] = 0"):
        _capi.linkage_codes(ok, [1, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="a total weight of 65537: at most 65536"):
        _capi.linkage_codes(ok, [65533, 1, 1, 1, 1])
    assert _capi.linkage_codes(ok, [65532, 1, 1, 1, 1])["size"][-1] == 65536
    with pytest.raises(ValueError, match="7 pairs are not the triangle"):
        _capi.linkage_codes(np.ones(7, dtype=np.int32))
    with pytest.raises(ValueError, match="method must be one of"):
        _capi.linkage_codes(ok, method="ward")
    with pytest.raises(ValueError, match="weights must hold one value per object"):
        _capi.linkage_codes(ok, [1, 1])
    with pytest.raises(ValueError, match="device must be -1"):
        _capi.linkage_codes(ok, device=-2)
    # the C checks behind the binding's own
    L, bad = _capi.load(), np.array([1, 2, -7], dtype=np.int32)
    out = np.zeros(2, dtype=_capi.LINKAGE_ROW)
    assert L.st_linkage_codes(-1, bad.ctypes.data, 3, None, 0, out.ctypes.data) == _capi.ST_ERR_ARG and _capi.last_error() == "codes[2] = -7 is negative"
    w = np.array([1, 0, 1], dtype=np.int32)
    assert L.st_linkage_codes(-1, np.abs(bad).ctypes.data, 3, w.ctypes.data, 0, out.ctypes.data) == _capi.ST_ERR_ARG
    assert _capi.last_error() == "weights[1] = 0: at least 1"
    assert L.st_linkage_codes(-1, bad.ctypes.data, 3, None, 5, out.ctypes.data) == _capi.ST_ERR_ARG and _capi.last_error().startswith("method 5")
    sq = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]])
    for value, message in ((np.nan, r"d\[2\]\[1\] = nan is not finite"), (np.inf, r"d\[2\]\[1\] = inf is not finite"), (-1.0, r"d\[2\]\[1\] = -1.0 is negative")):
        m = sq.copy()
        m[2, 1] = m[1, 2] = value
        with pytest.raises(ValueError, match=message):
            compare.linkage(m, device=None)
    m = sq.copy()
    m[2, 0] = 9.0
    with pytest.raises(ValueError, match="d is not symmetric"):
        compare.linkage(m, device=None)
    with pytest.raises(ValueError, match=r"d\[1\] = -2.0 is negative"):
        compare.linkage([1.0, -2.0, 3.0], device=None)
    with pytest.raises(ValueError, match="method must be one of"):
        compare.linkage(sq, "ward", device=None)
    with pytest.raises(ValueError, match="n = 1 objects"):
        compare.linkage(np.zeros((1, 1)), device=None)
    assert compare.linkage([2.5], device=None).heights.tolist() == [2.5]


def test_the_symbol_is_declared_and_exported():
    assert "st_linkage_codes" in _capi.SYMBOLS and hasattr(_capi.load(), "st_linkage_codes")
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    assert "int st_linkage_codes(int device" in header and "#define ST_API_VERSION 7" in header
    assert _capi.LINKAGE_MAX_OBJECTS == 16384 and _capi.LINKAGE_MAX_WEIGHT == 65536 and compare.LINKAGE_METHODS == tuple(_capi.LINKAGE_METHODS)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_linkage_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_linkage")
    csrc = os.path.join(ROOT, "suchtree_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "sanitize_linkage.cpp"), os.path.join(csrc, "linkage_plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "sanitize linkage ok" in out.stdout
