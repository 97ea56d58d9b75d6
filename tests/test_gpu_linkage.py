"""st_linkage_codes on the device (GPU): every result byte for byte that of the host restatement (device = -1), which the
CPU tests hold against the naive reference.  The chain is one workgroup of 1024 threads = 16 waves of 64: n = 2, 3 stay
inside a wave, 64 / 65 cross its edge, 1023 / 1024 / 1025 the workgroup's, 2049 gives a thread three rows and puts the
triangle index past 2^21.  Both homes of the cache (LDS, global) are forced through SUCHTREE_AMD_LINKAGE_CACHE.  Then the
facades: the dendrogram of the partner sets and the topology test, device against host."""
import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from linkage_reference import random_codes
from suchtree_amd import SuchLinkedTrees, SuchTree, _capi, compare

pytestmark = pytest.mark.gpu


def _same(codes, weights=None, method="average"):
    want = _capi.linkage_codes(codes, weights, method, -1)
    got = _capi.linkage_codes(codes, weights, method, 0)
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        t = int(np.flatnonzero(got != want)[0])
        raise AssertionError("row %d of %d: device %s, host %s" % (t, len(got), got[t], want[t]))
    return got


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1023, 1024, 1025, 2049])
def test_average_at_the_wave_and_workgroup_edges(n):
    rows = _same(random_codes(n, 100 + n))
    assert len(rows) == n - 1 and rows["size"][-1] == n


@pytest.mark.parametrize("n", [65, 1025])
@pytest.mark.parametrize("method", ["single", "complete"])
def test_single_and_complete(n, method):
    _same(random_codes(n, 200 + n), method=method)


@pytest.mark.parametrize("method", ["average", "single", "complete"])
def test_ties(method):
    rng = np.random.default_rng(7)
    _same(rng.integers(1, 4, size=300 * 299 // 2), method=method)
    _same(rng.integers(0, 2, size=300 * 299 // 2), method=method)
    rows = _same(np.full(130 * 129 // 2, 5), method=method)
    assert rows["left"].tolist() == [0] + list(range(2, 130)) and rows["right"].tolist() == [1] + list(range(130, 258))
    assert (rows["num"] == 5 * rows["den"]).all()


def test_weights():
    # sums of 60 bits, cross products of 89: a 64-bit comparison gets these wrong
    _same(np.array([2 ** 31 - 1 - k for k in range(28)]), [8192] * 8)
    rng = np.random.default_rng(11)
    for method in ("average", "single", "complete"):
        _same(random_codes(70, 3), rng.integers(1, 900, size=70), method)
        _same(rng.integers(1, 4, size=70 * 69 // 2), rng.integers(1, 4, size=70), method)


@pytest.mark.parametrize("n", [65, 1025])
@pytest.mark.parametrize("cache", ["lds", "global"])
def test_both_homes_of_the_cache(n, cache, monkeypatch):
    monkeypatch.setenv("SUCHTREE_AMD_LINKAGE_CACHE", cache)
    for method in ("average", "complete"):
        _same(random_codes(n, 300 + n), method=method)
    _same(np.random.default_rng(n).integers(1, 4, size=n * (n - 1) // 2))


def test_arguments_are_checked_before_the_device():
    with pytest.raises(ValueError, match="device 99 of"):
        _capi.linkage_codes(random_codes(5, 1), device=99)
    with pytest.raises(ValueError, match=r"weights\[1\] = 0"):
        _capi.linkage_codes(random_codes(3, 1), [1, 0, 1], device=0)


def _slt(which):
    d = golden_path(which)
    names = ("gopher.tree", "lice.tree") if which == "gopher_louse" else ("host.tree", "guest.tree")
    links = pd.read_csv(d + "/links.csv", index_col=0)
    return SuchLinkedTrees(SuchTree(d + "/" + names[0]), SuchTree(d + "/" + names[1]), links)


DENDROGRAM = ("left", "right", "size", "num", "den", "heights", "Z")
RESULT = ("rf", "rf_normalised", "exact", "n_a", "n_b", "transfer_total", "mean_transfer", "n_le", "transfer_n_le", "p_value", "transfer_p_value",
          "linkage", "rooted", "permutations", "seed", "stream", "measure", "names")


def _same_dendrogram(a, b):
    assert (a.n, a.method, a.shift) == (b.n, b.method, b.shift)
    for k in DENDROGRAM:
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k


@pytest.mark.parametrize("which", ["gopher_louse", "fish_worm"])
@pytest.mark.parametrize("linkage", ["average", "complete"])
def test_facades_agree_on_device_and_host(which, linkage):
    slt = _slt(which)
    before = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    parts = slt.partner_unifrac(of="A")
    dev = slt.partner_dendrogram(of="A", linkage=linkage, device=0)
    host = slt.partner_dendrogram(of="A", linkage=linkage, device=None)
    _same_dendrogram(dev, host)
    _same_dendrogram(dev, compare.linkage(np.asarray(parts.unifrac, dtype=np.float64), linkage, device=0))
    assert dev.leaves.tolist() == parts.leaves.tolist() and dev.names == parts.names and dev.measure == "unifrac" and dev.n == len(parts.leaves)
    kw = dict(of="A", linkage=linkage, permutations=99, seed=13, keep_stats=True, min_branch=0.0)
    got = slt.phylosymbiosis_topology(device=0, **kw)
    want = slt.phylosymbiosis_topology(device=None, **kw)
    for k in RESULT:
        va, vb = getattr(got, k), getattr(want, k)
        assert va == vb or (va != va and vb != vb), k
    for k in ("perm_rf", "perm_transfer", "leaves"):
        va, vb = getattr(got, k), getattr(want, k)
        assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), k
    _same_dendrogram(got.dendrogram, want.dendrogram)
    assert got.matches.distance.tolist() == want.matches.distance.tolist() and got.matches.match.tolist() == want.matches.match.tolist()
    assert got.n_le == int((got.perm_rf <= got.rf).sum()) and got.p_value == (got.n_le + 1) / 100
    stat, p, n = got
    assert (stat, p, n) == (got.rf, got.p_value, dev.n)
    # the tree's own facade over the same rows
    mine = slt.TreeA.dendrogram_congruence(np.asarray(parts.unifrac, dtype=np.float64), parts.leaves, linkage=linkage, permutations=99, seed=13,
                                           keep_stats=True, min_branch=0.0, device=0)
    assert mine.perm_rf.tolist() == got.perm_rf.tolist() and mine.rf == got.rf and mine.measure is None
    after = (np.array(slt.subset_a_leafs), np.array(slt.subset_b_leafs), np.array(slt.linklist))
    assert all((p == q).all() for p, q in zip(before, after))
