"""Every clade at once without a GPU: the clade plan of st_clade_plan against brute force, argument errors, the
CladeComparisons table and its p-values, the exports, and the registers of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
from scipy.stats import pearsonr

from conftest import ROOT, golden_path
from suchtree_amd import SuchTree, _capi, build as st_build, synth
from suchtree_amd.compare import CladeComparisons, DistanceComparison, pearson_pvalue
from suchtree_amd.linked import SuchLinkedTrees


@pytest.fixture(scope="module")
def lib():
    st_build.build()
    return _capi.load()


def _children(parent):
    ch = {v: [] for v in range(len(parent))}
    for v, p in enumerate(parent):
        if p >= 0:
            ch[int(p)].append(v)
    return ch


def _subtree(ch, v):
    out, todo = [], [v]
    while todo:
        u = todo.pop()
        out.append(u)
        todo.extend(ch[u])
    return out


def _segment_pairs(seg, perm):
    """The (lower rank, higher rank) pairs of one segment, in its pair order."""
    if seg["kind"] == _capi.CLADE_RECT:
        pos = [(p, q) for p in range(seg["row_begin"], seg["row_end"]) for q in range(seg["col_begin"], seg["col_end"])]
    else:
        pos = [(seg["row_begin"] + j, seg["row_begin"] + i) for i in range(1, seg["row_end"] - seg["row_begin"]) for j in range(i)]
    return [tuple(sorted((int(perm[p]), int(perm[q])))) for p, q in pos]


def _check_plan(parent, leaf_of_link, max_links=None):
    plan = _capi.clade_plan(parent, leaf_of_link, max_links=max_links)
    n, L = len(parent), len(leaf_of_link)
    ch = _children(parent)
    perm, begin, count, segs = plan["perm"], plan["begin"], plan["count"], plan["segments"]
    assert sorted(perm.tolist()) == list(range(L))
    assert np.all(np.diff(segs["first_pair"]) == segs["n_pairs"][:-1]) and (len(segs) == 0 or segs["first_pair"][0] == 0)
    assert plan["total_pairs"] == int(segs["n_pairs"].sum())
    assert np.all(segs["n_pairs"] > 0)
    seg_by_node = {}
    for s in segs:
        assert len(_segment_pairs(s, perm)) == s["n_pairs"]
        seg_by_node.setdefault(int(s["node"]), []).append(s)
    want_total = 0
    for v in range(n):
        under = set(_subtree(ch, v))
        links = [j for j in range(L) if int(leaf_of_link[j]) in under]
        assert count[v] == len(links)
        assert sorted(perm[begin[v]:begin[v] + count[v]].tolist()) == links      # one contiguous range
        assert plan["leaves"][v] == sum(1 for u in under if not ch[u])
        capped = max_links is not None and count[v] > max_links
        if capped:
            assert v not in seg_by_node
            continue
        want = sorted((links[j], links[i]) for i in range(len(links)) for j in range(i))
        got = sorted(p for u in under for s in seg_by_node.get(u, []) for p in _segment_pairs(s, perm))
        assert got == want, v      # every pair once, oriented (lower rank, higher rank)
        own = sum(int(s["n_pairs"]) for s in seg_by_node.get(v, []))
        want_total += own
    assert plan["total_pairs"] == want_total
    return plan


def _links(parent, rng, top=3):
    leaves = [v for v, c in _children(parent).items() if not c]
    mult = rng.integers(0, top + 1, len(leaves))
    out = np.repeat(np.array(leaves, dtype=np.int64), mult)
    return out[rng.permutation(len(out))]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_random_binary_against_brute_force(lib, seed):
    rng = np.random.default_rng(seed)
    parent, _ = synth.random_binary_tree(40 + 10 * seed, seed=seed)
    links = _links(parent, rng)
    plan = _check_plan(parent, links)
    assert plan["total_pairs"] == len(links) * (len(links) - 1) // 2
    for cap in (0, 3, 10, len(links) - 1):
        _check_plan(parent, links, max_links=cap)


def test_plan_complete_tree_and_caterpillar(lib):
    rng = np.random.default_rng(5)
    parent, _ = synth.complete_tree(37)
    _check_plan(parent, _links(parent, rng))
    _check_plan(parent, _links(parent, rng), max_links=6)
    # a deep caterpillar: iterative plan, checked on counts and the pair total (the brute force above is O(n^2))
    parent, _ = synth.caterpillar_tree(5000)
    links = _links(parent, rng)
    plan = _capi.clade_plan(parent, links)
    root = int(np.flatnonzero(parent == -1)[0])
    assert plan["count"][root] == len(links) and plan["total_pairs"] == len(links) * (len(links) - 1) // 2
    capped = _capi.clade_plan(parent, links, max_links=100)
    keep = set(np.flatnonzero(plan["count"] <= 100).tolist())
    assert set(capped["segments"]["node"].tolist()) <= keep
    assert capped["total_pairs"] == sum(int(s["n_pairs"]) for s in plan["segments"] if int(s["node"]) in keep)
    # 1e5 levels do not recurse
    parent, _ = synth.caterpillar_tree(100_000)
    assert _capi.clade_plan(parent, np.arange(0, 2 * 100_000 - 1, 2, dtype=np.int64))["total_pairs"] == 100_000 * 99_999 // 2


def test_plan_and_clade_errors_without_a_gpu(lib):
    parent, _ = synth.random_binary_tree(20, seed=1)
    internal = int(np.flatnonzero(parent == -1)[0])
    with pytest.raises(ValueError):           # not a leaf
        _capi.clade_plan(parent, np.array([0, internal], dtype=np.int64))
    with pytest.raises(_capi.InvalidNodeError):
        _capi.clade_plan(parent, np.array([0, len(parent) + 3], dtype=np.int64))
    with pytest.raises(_capi.InvalidNodeError):
        _capi.clade_plan(parent, np.array([-1, 0], dtype=np.int64))
    bad = parent.copy()
    bad[0] = -1                               # two roots
    with pytest.raises(_capi.TreeStructureError):
        _capi.clade_plan(bad, np.array([2], dtype=np.int64))
    # st_compare_clades_host checks its arguments before it touches a tree: NULL trees, a bad chunk size
    out = np.zeros(len(parent), dtype=_capi.PAIR_MOMENTS)
    ids = np.array([0, 2], dtype=np.int64)
    b = ctypes.c_int64(0)
    p32 = np.ascontiguousarray(parent, dtype=np.int32)
    rc = lib.st_compare_clades_host(None, None, _capi._ptr(p32), len(parent), _capi._ptr(ids), _capi._ptr(ids), 2, -1, 0,
                                    _capi._ptr(out), None, ctypes.byref(b))
    assert rc == _capi.ST_ERR_ARG
    rc = lib.st_compare_clades_host(None, None, _capi._ptr(p32), len(parent), _capi._ptr(ids), _capi._ptr(ids), 2, -1, 0, None,
                                    None, ctypes.byref(b))
    assert rc == _capi.ST_ERR_ARG


def test_clade_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "suchtree_hip.h")).read()
    for name in ("st_clade_plan", "st_compare_clades_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS
        assert getattr(lib, name) is not None
    assert "typedef struct st_clade_segment" in header
    assert re.search(r"#define ST_CLADE_TILE\s+%d\b" % _capi.CLADE_TILE, header)
    assert _capi.CLADE_SEGMENT.itemsize == 40 and _capi.PAIR_MOMENTS.itemsize == ctypes.sizeof(_capi.PairMoments)
    assert lib.st_api_version() == 7 == _capi.API_VERSION


def _table(rng, k=50):
    """A CladeComparisons over k hand-built rows: sums of random columns about random shifts."""
    rows, data = [], []
    for i in range(k):
        n_links = int(rng.integers(3, 40))
        m = n_links * (n_links - 1) // 2
        x = rng.normal(3, 1, m)
        y = 0.5 * x + rng.normal(0, 1, m)
        if i == 3:
            x[:] = 2.0                        # a constant column: NaN r
        cx, cy = x[0], y[0]
        rows.append((n_links, cx, cy, (x - cx).sum(), (y - cy).sum(), ((x - cx) ** 2).sum(), ((y - cy) ** 2).sum(),
                     ((x - cx) * (y - cy)).sum(), x.min(), x.max(), y.min(), y.max()))
        data.append((x, y))
    a = np.array(rows)
    sums = {k: a[:, i + 1] for i, k in enumerate(("shift_x", "shift_y", "sx", "sy", "sxx", "syy", "sxy"))}
    nodes = np.arange(100, 100 + k)
    return CladeComparisons(nodes, a[:, 0].astype(np.int64) + 1, a[:, 0].astype(np.int64), sums, a[:, 8], a[:, 9], a[:, 10],
                            a[:, 11]), data


def test_comparison_and_dataframe_on_hand_built_sums():
    C, data = _table(np.random.default_rng(1))
    assert len(C) == 50
    for i, (x, y) in enumerate(data):
        c = C.comparison(100 + i)
        assert isinstance(c, DistanceComparison)
        assert c.n_pairs == len(x) == C.n_pairs[i] and c.n_leaves == C.n_links[i]
        for col, attr in (("mean_a", "mean_x"), ("mean_b", "mean_y"), ("var_a", "var_x"), ("var_b", "var_y"), ("cov", "cov"),
                          ("pearson_r", "pearson_r")):
            assert np.array_equal(getattr(C, col)[i], getattr(c, attr), equal_nan=True), (i, col)
        assert abs(c.mean_x - x.mean()) < 1e-12 and abs(c.var_y - y.var()) < 1e-10
        if i == 3:
            assert np.isnan(c.pearson_r) and np.isnan(C.pvalue[i])
        else:
            assert abs(c.pearson_r - np.corrcoef(x, y)[0, 1]) < 1e-12
    with pytest.raises(KeyError):
        C.comparison(7)
    df = C.to_dataframe()
    assert list(df.columns[:5]) == ["name", "n_links", "n_leafs", "r", "p"]
    assert df["name"][0] == "clade_100" and len(df) == 50
    assert np.array_equal(df["r"].to_numpy(), C.pearson_r, equal_nan=True)
    assert np.array_equal(df["n_leafs"].to_numpy(), C.n_leaves)


def test_pvalue_matches_scipy_pearsonr():
    rng = np.random.default_rng(2)
    rs, ns, want = [], [], []
    for n in list(range(2, 12)) + [50, 300, 5000]:
        for _ in range(4):
            x = rng.normal(size=n)
            y = 0.3 * x + rng.normal(size=n)
            res = pearsonr(x, y)
            rs.append(res[0])
            ns.append(n)
            want.append(res[1])
    got = pearson_pvalue(np.array(rs), np.array(ns))
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-9 * abs(w) + 1e-300, (g, w)
    assert np.isnan(pearson_pvalue(np.array([np.nan]), np.array([10]))[0])
    assert np.isnan(pearson_pvalue(np.array([0.5]), np.array([1]))[0])


def test_rank_order_matches_the_root_linklist():
    d = golden_path("gopher_louse")
    S = SuchLinkedTrees(SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree"), pd.read_csv(d + "/links.csv", index_col=0))
    A, B = S.TreeA, S.TreeB
    for v in B.get_internal_nodes()[:6]:
        assert np.array_equal(S._leaf_order(B, v), S._leaves_below(B, v))
    for T in (A, B, SuchTree(synth.caterpillar_tree(300))):
        assert np.array_equal(S._breadth_first(T, T.root_node, False), T.get_internal_nodes())
    col_of = np.full(B.size, -1, dtype=np.int64)
    col_of[S._col_ids] = np.arange(len(S._col_ids))
    got = S._links_in_order(col_of[S._leaf_order(B, B.root_node)], S._subset_a_leafs)
    before = S.linklist.copy()
    S.subset_b(B.root_node)
    assert np.array_equal(got[0], S.linklist[:, 1]) and np.array_equal(got[1], S.linklist[:, 0])
    assert not np.array_equal(before, S.linklist)      # (the default order is the table's, not the root's)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_clade_kernels_compile_for_gfx950_without_spills(tmp_path):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-DST_CANOPY_PART=3", "-o", str(tmp_path / "unit.o"),
                          os.path.join(ROOT, "suchtree_amd", "csrc", "launch_canopy.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "SrcSegments" in out.stderr
    for m in re.finditer(r"VGPRs Spill: (\d+)", out.stderr):
        assert int(m.group(1)) == 0
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "main.o"), os.path.join(ROOT, "suchtree_amd", "csrc", "suchtree_hip.hip")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    name, seen = None, False
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name and "k_clade_pieces" in name:
            seen = True
            assert int(m.group(1)) == 0
    assert seen
