"""The order in which the eight two-tree compare entry points report argument errors, through raw ctypes, and the
sequence of library calls SuchTree.compare_distances / SuchLinkedTrees.linked_distances_summary make.

Every entry point checks, in this order: (1) its outputs (the histogram arguments first), (2) the trees, (3) the range of
its input, (4) the chunk size, (5) the pair count, where ranks and Kendall counts bound it, (6) the NULL id arrays.  Each
row below violates two neighbouring rungs at once and names the message of the earlier one.  Rows that need a tree handle
run on the GPU, over a 16-leaf tree."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from conftest import golden_path
from suchtree_amd import SuchTree, _capi, build as st_build, synth
from suchtree_amd.linked import SuchLinkedTrees

LIVE = "live"                      # stands for a tree handle in a row
TWO31 = 1 << 31                    # one pair more than ranks and Kendall counts take
IDS = np.arange(0, 32, 2, dtype=np.int64)      # the 16 leaves of balanced_tree(4): 120 pairs, 1820 quartets
ROWS = np.zeros((3, 4), dtype=np.int64)        # three explicit pairs (its first 12 values) or quartets
EDGES = np.linspace(0.0, 1.0, 9)
HIST = np.zeros(64, dtype=np.int64)

_TRI = dict(x=IDS, y=IDS, m=16, k_begin=0, k_count=120)
_PRS = dict(x=ROWS, y=ROWS, n=3)
_HIST = dict(edges_x=None, bins_x=0, edges_y=None, bins_y=0)
# entry point -> its arguments in order with valid values; "out", "out2" and "hist" are filled in per call
ENTRIES = {
    "st_compare_triangle_host": dict(_TRI, **_HIST, out=True, hist=None),
    "st_compare_pairs_host": dict(_PRS, **_HIST, out=True, hist=None),
    "st_compare_triangle_ranks_host": dict(_TRI, chunk=0, out=True, out2=True),
    "st_compare_pairs_ranks_host": dict(_PRS, chunk=0, out=True, out2=True),
    "st_compare_triangle_kendall_host": dict(_TRI, chunk=0, out=True, out2=True),
    "st_compare_pairs_kendall_host": dict(_PRS, chunk=0, out=True, out2=True),
    "st_compare_quartets_leaves_host": dict(x=IDS, y=IDS, m=16, mode=0, seed=0, k_begin=0, k_count=1820, chunk=0, out=True),
    "st_compare_quartets_host": dict(_PRS, chunk=0, out=True),
}
MOMENTS = [e for e in ENTRIES if e in ("st_compare_triangle_host", "st_compare_pairs_host")]
RANKED = [e for e in ENTRIES if "ranks" in e or "kendall" in e]
QUARTETS = [e for e in ENTRIES if "quartets" in e]
TRIANGLES = [e for e in ENTRIES if "triangle" in e]
NULL_OUT = {e: "out is NULL" for e in MOMENTS + QUARTETS}
NULL_OUT.update({e: "out or out_ranks is NULL" for e in RANKED if "ranks" in e})
NULL_OUT.update({e: "out or out_counts is NULL" for e in RANKED if "kendall" in e})
NULL_IDS = {e: "ids_x or ids_y is NULL" for e in TRIANGLES + ["st_compare_quartets_leaves_host"]}
NULL_IDS.update({e: "pairs_x or pairs_y is NULL" for e in ENTRIES if "pairs" in e})
NULL_IDS["st_compare_quartets_host"] = "quartets_x or quartets_y is NULL"
TREES = "tree_x or tree_y is NULL"
HIST_ARGS = "edges_x, edges_y and out_hist must all be given or all be NULL"
CHUNK_PAIRS = "chunk_pairs must be 0 or a positive multiple of"
CHUNK_QUARTETS = "chunk_quartets must be 0 or a positive value of at most"
# the first range error of each input, with the arguments that provoke it
BAD_RANGE = {e: (dict(m=-1), "negative size") for e in TRIANGLES}
BAD_RANGE.update({e: (dict(n=-1), "n < 0") for e in ENTRIES if e not in TRIANGLES})
BAD_RANGE["st_compare_quartets_leaves_host"] = (dict(mode=7), "mode must be ST_QUARTET_ALL or ST_QUARTET_SAMPLE")
# 2^31 pairs: a range that holds them (70,000 leaves have 2,449,965,000 pairs)
TOO_MANY = {e: dict(m=70000, k_count=TWO31) if e in TRIANGLES else dict(n=TWO31) for e in RANKED}
COUNT = {e: ("ranks of %d pairs: at most" if "ranks" in e else "Kendall counts of %d pairs: at most") % TWO31 for e in RANKED}


def _rows():
    def row(entry, what, over, want, trees=(None, None)):
        live = LIVE in trees
        return pytest.param(entry, dict(over), want, trees, id="%s-%s" % (entry[len("st_compare_"):-len("_host")] or "triangle", what),
                            marks=[pytest.mark.gpu] if live else [])

    for e in ENTRIES:
        # 1 before 2: a NULL output and NULL trees
        yield row(e, "out-before-trees", dict(out=None), NULL_OUT[e])
        yield row(e, "trees", {}, TREES)
        # 2 before 3: a NULL tree_y and a bad range
        yield row(e, "trees-before-range", BAD_RANGE[e][0], TREES, (LIVE, None))
        # 6, alone: everything above it holds
        yield row(e, "null-ids", dict(x=None, y=None), NULL_IDS[e], (LIVE, LIVE))
    for e in MOMENTS:
        # within 1: the histogram arguments before `out`, and before the trees
        yield row(e, "hist-before-out", dict(edges_x=EDGES, bins_x=8, edges_y=EDGES, bins_y=8, out=None), HIST_ARGS)
        yield row(e, "hist-before-trees", dict(edges_x=EDGES, bins_x=8, hist=HIST), HIST_ARGS)
    # 3 before 6 where there is neither 4 nor 5: a range beyond the triangle and NULL ids
    yield row("st_compare_triangle_host", "range-before-null-ids", dict(k_count=121, x=None, y=None), "pair range exceeds m(m-1)/2", (LIVE, LIVE))
    for e in RANKED + QUARTETS:
        # 3 before 4: a bad range and a bad chunk
        yield row(e, "range-before-chunk", dict(BAD_RANGE[e][0], chunk=-1), BAD_RANGE[e][1], (LIVE, LIVE))
    for e in RANKED:
        # 4 before 5: a chunk that is no multiple of the tile and 2^31 pairs; 5 before 6: 2^31 pairs and NULL ids
        yield row(e, "chunk-before-count", dict(TOO_MANY[e], chunk=1), CHUNK_PAIRS, (LIVE, LIVE))
        yield row(e, "count-before-null-ids", dict(TOO_MANY[e], x=None, y=None), COUNT[e], (LIVE, LIVE))
    for e in QUARTETS:
        # 4 before 6 (quartets have no 5): a negative chunk and NULL ids
        yield row(e, "chunk-before-null-ids", dict(chunk=-1, x=None, y=None), CHUNK_QUARTETS, (LIVE, LIVE))


@pytest.fixture(scope="module")
def lib():
    st_build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def live():
    return _capi.DeviceTree(*synth.balanced_tree(4))


@pytest.mark.parametrize("entry,over,want,trees", list(_rows()))
def test_the_earlier_rung_is_reported(lib, request, entry, over, want, trees):
    args = dict(ENTRIES[entry], **over)
    results = {"st_compare_triangle_ranks_host": _capi.RankSums, "st_compare_pairs_ranks_host": _capi.RankSums,
               "st_compare_triangle_kendall_host": _capi.KendallCounts, "st_compare_pairs_kendall_host": _capi.KendallCounts}
    out = (_capi.QuartetTable if entry in QUARTETS else _capi.PairMoments)()
    out2 = results[entry]() if entry in results else None
    bad = ctypes.c_int64(0)
    handles = [request.getfixturevalue("live").handle if t == LIVE else None for t in trees]
    argv = []
    for k, v in args.items():
        if k == "out":
            argv.append(ctypes.byref(out) if v else None)
        elif k == "out2":
            argv.append(ctypes.byref(out2) if v else None)
        elif isinstance(v, np.ndarray):
            argv.append(v.ctypes.data_as(ctypes.c_void_p))
        else:
            argv.append(v)
    assert getattr(lib, entry)(*handles, *argv, ctypes.byref(bad)) == _capi.ST_ERR_ARG
    assert want in _capi.last_error(), _capi.last_error()


# ---- the calls behind compare_distances and linked_distances_summary ------------------------------------------------
class StubTree:
    """Stands in for _capi.DeviceTree: records which compare method ran and whether it was given edges."""

    def __init__(self, log):
        self.log = log

    def _moments(self):
        m = _capi.PairMoments()
        m.n, m.min_x, m.max_x, m.min_y, m.max_y = 6, 0.0, 1.0, 0.0, 2.0
        return m

    def _record(self, name, second):
        def method(other, a, b, edges="-", **kw):
            assert isinstance(other, StubTree)
            self.log.append(name if edges == "-" else "%s(%s)" % (name, "None" if edges is None else "edges"))
            return self._moments(), second(edges)
        return method

    def __getattr__(self, name):
        if name in ("compare_triangle_host", "compare_pairs_host"):
            return self._record(name, lambda edges: None if edges is None else np.zeros((len(edges[0]) - 1, len(edges[1]) - 1), np.int64))
        if name in ("compare_triangle_ranks_host", "compare_pairs_ranks_host"):
            return self._record(name, lambda _: _capi.RankSums())
        if name in ("compare_triangle_kendall_host", "compare_pairs_kendall_host"):
            return self._record(name, lambda _: _capi.KendallCounts())
        raise AttributeError(name)


# (bins, spearman, kendall) -> the calls, as the parent of the commit that introduced this table made them; %s is
# "triangle" or "pairs"
CALLS = {
    ("none", False, False): ["compare_%s_host(None)"],
    ("none", True, False): ["compare_%s_ranks_host"],
    ("none", False, True): ["compare_%s_kendall_host"],
    ("none", True, True): ["compare_%s_kendall_host", "compare_%s_ranks_host"],
    ("int", False, False): ["compare_%s_host(None)", "compare_%s_host(edges)"],
    ("int", True, False): ["compare_%s_ranks_host", "compare_%s_host(None)", "compare_%s_host(edges)"],
    ("int", False, True): ["compare_%s_kendall_host", "compare_%s_host(None)", "compare_%s_host(edges)"],
    ("int", True, True): ["compare_%s_kendall_host", "compare_%s_ranks_host", "compare_%s_host(None)", "compare_%s_host(edges)"],
    ("edges", False, False): ["compare_%s_host(edges)"],
    ("edges", True, False): ["compare_%s_ranks_host", "compare_%s_host(edges)"],
    ("edges", False, True): ["compare_%s_kendall_host", "compare_%s_host(edges)"],
    ("edges", True, True): ["compare_%s_kendall_host", "compare_%s_ranks_host", "compare_%s_host(edges)"],
}
BINS = {"none": None, "int": 4, "edges": (np.linspace(0, 1, 5), np.linspace(0, 2, 4))}


def _stubbed(monkeypatch):
    log = []
    monkeypatch.setattr(SuchTree, "_device_tree", lambda self: StubTree(log))
    return log


@pytest.mark.parametrize("bins,spearman,kendall", list(CALLS))
def test_library_calls_of_compare_distances_and_linked_summary(monkeypatch, bins, spearman, kendall):
    log = _stubbed(monkeypatch)
    a, b = SuchTree(synth.balanced_tree(4)), SuchTree(synth.balanced_tree(4, seed=1))
    pairs = (np.array([[0, 2], [4, 6]]), np.array([[2, 4], [0, 6]]))
    d = golden_path("gopher_louse")
    slt = SuchLinkedTrees(SuchTree(d + "/gopher.tree"), SuchTree(d + "/lice.tree"), pd.read_csv(d + "/links.csv", index_col=0))
    for kind, call in (("triangle", lambda **kw: a.compare_distances(b, leaves=(IDS, IDS), **kw)),
                       ("pairs", lambda **kw: a.compare_distances(b, pairs=pairs, **kw)),
                       ("triangle", lambda **kw: slt.linked_distances_summary(**kw))):
        del log[:]
        c = call(bins=BINS[bins], spearman=spearman, kendall=kendall)
        assert log == [s % kind for s in CALLS[(bins, spearman, kendall)]], (kind, log)
        assert (c.hist is None) == (bins == "none") and (c.rank_sxy is None) != spearman and (c.discordant is None) != kendall
        assert c.n_pairs == 6 and (c.n_leaves is None) == (kind == "pairs")
