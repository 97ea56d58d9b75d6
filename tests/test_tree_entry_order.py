"""The order in which the one-tree entry points report argument errors, through raw ctypes, and the rule of every handle
option of st_tree_set_option.

Each row of the first table violates two neighbouring rungs of an entry point's ladder of checks at once (or its last rung
alone) and names the exact message of the earlier one.  The rungs above the first use of the handle never look into it:
their rows pass a block of zeroed memory for the tree and run without a GPU.  The others are marked gpu and use the handle
of a 16-leaf tree.  One call per row and no kernel of any size."""
import ctypes

import numpy as np
import pytest

from suchtree_amd import _capi, build as st_build, synth

LIVE = "live"                      # a real tree handle
STUB = "stub"                      # zeroed memory: enough for rungs that only ask whether the pointer is NULL
_STUB_MEMORY = ctypes.create_string_buffer(1 << 20)
I64 = np.arange(0, 32, 2, dtype=np.int64)      # the 16 leaves of balanced_tree(4); also three (n,2) pairs, four quartets
I32 = np.arange(0, 32, 2, dtype=np.int32)
F64 = np.zeros(256, dtype=np.float64)
OUT = np.zeros(256, dtype=np.int64)            # any output array: no row gets as far as writing it
BAD_EDGE = np.array([0, 9], dtype=np.int32)    # an endpoint beyond n = 4
W2 = np.ones(2, dtype=np.float64)
BIG = 3000000001

_PAIRS = dict(t=STUB, pairs=I64, n=3, s0=2, s1=1, out_d=OUT, out_m=OUT, last=0)
_TRI = dict(t=STUB, ids=I64, m=16, id_stride=1, k_begin=0, k_count=120, out_d=OUT, out_m=OUT, last=0)
# entry point -> its arguments in order, with valid values ("last" is bad_id or the stream)
ENTRIES = {
    "st_distances_host": _PAIRS,
    "st_distances_host_i32": dict(_PAIRS, pairs=I32),
    "st_distances_device": _PAIRS,
    "st_distances_device_f32": _PAIRS,
    "st_distances_device_wire": _PAIRS,
    "st_unpack_mrca24_device": dict(device=0, packed=OUT, n=3, out=OUT, last=0),
    "st_triangle_host": _TRI,
    "st_triangle_device": _TRI,
    "st_grid_host": dict(t=STUB, rows=I64, n_rows=4, cols=I64, n_cols=4, symmetric=0, e_begin=0, e_count=16, out_d=OUT, out_m=OUT, last=0),
    "st_knn_host": dict(t=STUB, queries=I64, n_queries=2, cands=I64, n_cands=2, k=1, skip_self=0, out_i=OUT, out_d=F64, last=0),
    "st_quartets_host": dict(t=STUB, quartets=I64, n=4, s0=4, s1=1, out=OUT, last=0),
    "st_graph_matrices_host": dict(device=0, n=4, n_edges=2, u=I32, v=I32, w=W2, out_a=F64, out_l=F64),
    "st_tree_set_option": dict(t=STUB, name=b"wire24", value=1),
}
HOST_BAD_ID = ("st_distances_host", "st_distances_host_i32", "st_triangle_host", "st_grid_host", "st_knn_host", "st_quartets_host")
PAIR_ENTRIES = [e for e in ENTRIES if e.startswith("st_distances_")]
TRIANGLES = ("st_triangle_host", "st_triangle_device")
NO_OUT = dict(out_d=None, out_m=None)


def _rows():
    def row(entry, what, over, want):
        args = dict(ENTRIES[entry], **over)
        return pytest.param(entry, over, want, id="%s-%s" % (entry[3:], what), marks=[pytest.mark.gpu] if args.get("t") == LIVE else [])

    for e in PAIR_ENTRIES:      # tree, n, pairs, outputs
        yield row(e, "tree-before-n", dict(t=None, n=-1), "tree is NULL")
        yield row(e, "n-before-pairs", dict(n=-1, pairs=None), "n < 0")
        yield row(e, "pairs-before-outputs", dict(pairs=None, **NO_OUT), "pairs is NULL")
        yield row(e, "outputs", NO_OUT, "both outputs are NULL")
    # the 24-bit form's own rungs come behind those four and read the handle: a live one, an odd output address
    yield row("st_distances_device_wire", "outputs-before-alignment", dict(t=LIVE, out_d=None, out_m=None), "both outputs are NULL")
    yield row("st_distances_device_wire", "alignment", dict(t=LIVE, out_d=None, out_m=0x1002), "d_out_mrca24 must be 4-byte aligned")
    # n, buffers, then the device (99: there is none, and the row never gets there)
    yield row("st_unpack_mrca24_device", "n-before-buffers", dict(n=-1, packed=None, out=None), "n < 0")
    yield row("st_unpack_mrca24_device", "buffers-before-device", dict(device=99, packed=None), "buffer is NULL")
    for e in TRIANGLES:         # tree, the range (sizes, m, the triangle), ids, outputs
        yield row(e, "tree-before-range", dict(t=None, m=-1), "tree is NULL")
        yield row(e, "sizes-before-m", dict(k_begin=-1, m=BIG), "negative size")
        yield row(e, "m-before-ids", dict(m=BIG, ids=None), "m too large")
        yield row(e, "range-before-ids", dict(k_count=121, ids=None), "pair range exceeds m(m-1)/2")
        yield row(e, "ids-before-outputs", dict(ids=None, **NO_OUT), "ids is NULL")
        yield row(e, "outputs", NO_OUT, "both outputs are NULL")
    e = "st_grid_host"          # tree, sizes, size limit, element range, id lists, outputs, symmetry
    yield row(e, "tree-before-sizes", dict(t=None, n_rows=-1), "tree is NULL")
    yield row(e, "sizes-before-limit", dict(n_rows=-1, n_cols=BIG), "negative size")
    yield row(e, "limit-before-range", dict(n_rows=BIG, n_cols=0, e_count=1), "grid too large")
    yield row(e, "range-before-ids", dict(e_count=17, rows=None), "element range exceeds n_rows * n_cols")
    yield row(e, "ids-before-outputs", dict(cols=None, **NO_OUT), "id list is NULL")
    yield row(e, "outputs-before-symmetry", dict(symmetric=1, n_cols=3, e_count=12, **NO_OUT), "both outputs are NULL")
    yield row(e, "symmetry-after-range", dict(t=LIVE, symmetric=1, n_cols=3, e_count=12), "symmetric grid needs n_rows == n_cols")
    e = "st_knn_host"           # tree, sizes, k, candidate limit, queries and outputs, candidates
    yield row(e, "tree-before-sizes", dict(t=None, n_queries=-1), "tree is NULL")
    yield row(e, "sizes-before-k", dict(n_cands=-1, k=0), "negative size")
    yield row(e, "k-low-before-limit", dict(k=0, n_cands=1 << 32), "k must be in [1, 256]")
    yield row(e, "k-high-before-limit", dict(k=257, n_cands=1 << 32), "k must be in [1, 256]")
    yield row(e, "limit-before-queries", dict(n_cands=1 << 32, queries=None), "too many candidates")
    yield row(e, "queries-before-cands", dict(out_d=None, cands=None), "queries or output is NULL")
    yield row(e, "cands", dict(cands=None), "cands is NULL")
    e = "st_quartets_host"      # tree, n, quartets and output
    yield row(e, "tree-before-n", dict(t=None, n=-1), "tree is NULL")
    yield row(e, "n-before-arrays", dict(n=-1, quartets=None), "n < 0")
    yield row(e, "arrays", dict(out=None), "quartets or output is NULL")
    e = "st_graph_matrices_host"      # sizes, edge arrays, outputs, endpoints, then the device
    yield row(e, "sizes-before-edges", dict(n=0, u=None), "bad sizes")
    yield row(e, "edges-negative", dict(n_edges=-1, u=None), "bad sizes")
    yield row(e, "edges-before-outputs", dict(w=None, out_a=None, out_l=None), "edge arrays are NULL")
    yield row(e, "outputs-before-endpoints", dict(out_a=None, out_l=None, u=BAD_EDGE), "both outputs are NULL")
    yield row(e, "endpoints-before-device", dict(v=BAD_EDGE, device=99), "edge endpoint out of range")
    e = "st_tree_set_option"
    yield row(e, "null-tree", dict(t=None, name=b"nope"), "tree or name is NULL")
    yield row(e, "null-name", dict(name=None, value=9), "tree or name is NULL")
    yield row(e, "null-name-live", dict(t=LIVE, name=None), "tree or name is NULL")
    yield row(e, "unknown-before-value", dict(t=LIVE, name=b"nope", value=-5), "unknown option nope")


@pytest.fixture(scope="module")
def lib():
    st_build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def live():
    return _capi.DeviceTree(*synth.balanced_tree(4))


@pytest.mark.parametrize("entry,over,want", list(_rows()))
def test_the_earlier_rung_is_reported(lib, request, entry, over, want):
    args = dict(ENTRIES[entry], **over)
    bad = ctypes.c_int64(0)
    argv = []
    for k, v in args.items():
        if k == "t" and v == LIVE:
            argv.append(request.getfixturevalue("live").handle)
        elif k == "t" and v == STUB:
            argv.append(ctypes.cast(_STUB_MEMORY, ctypes.c_void_p))
        elif isinstance(v, np.ndarray):
            argv.append(v.ctypes.data_as(ctypes.c_void_p))
        elif k == "last":
            argv.append(ctypes.byref(bad) if entry in HOST_BAD_ID else None)
        else:
            argv.append(v)
    assert getattr(lib, entry)(*argv) == _capi.ST_ERR_ARG
    assert _capi.last_error() == want


# ---- the option rules ------------------------------------------------------------------------------------------------
ZERO_ONE = ("tile_sort", "ladder_scalar", "ladder_dynamic", "cherries", "batch_probe", "tree_rmq", "mrca_ranks", "rec_a4", "walk_ladder",
            "prefer_walk_sorted", "wire48", "wire24", "walk_crown", "walk_sort", "lineage_lens", "lineage_sums", "ladder_sums")
ZERO_TO_TWO = ("heap_lines", "heap_codes", "stream_hint")
NOT_NEGATIVE = ("ladder_min_pairs", "walk_sort_min")
MEASURE = "measure must be a combination of 1 (trace), 2 (skip CPU passes), 4 (skip GPU side)"
# what a 16-leaf tree's handle starts with (st_tree.h: a shallow tree, nothing timed when it is created)
DEFAULT = dict.fromkeys(ZERO_ONE + ZERO_TO_TWO, 1)
DEFAULT.update(dict.fromkeys(("tile_sort", "ladder_scalar", "prefer_walk_sorted", "ladder_sums", "sort_tile", "measure", "reserve_cus")
                             + NOT_NEGATIVE, 0), small_batch_path=1)
# option -> (accepted values: the lowest and the highest legal among them, refused values, the message)
RULES = {name: ((0, 1), (-1, 2), name + " must be 0 or 1") for name in ZERO_ONE}
RULES.update({name: ((0, 2), (-1, 3), name + " must be 0, 1 or 2") for name in ZERO_TO_TWO})
RULES.update({name: ((0, (1 << 63) - 1), (-1, -(1 << 63)), name + " must be >= 0") for name in NOT_NEGATIVE})
RULES["sort_tile"] = ((0, 1, 2, 4), (-1, 3, 5), "sort_tile must be 0, 1, 2 or 4")
RULES["measure"] = ((0, 7), (-1, 8), MEASURE)
RULES["small_batch_path"] = ((0, 1, 7, -1), (), None)


@pytest.fixture(scope="module")
def optioned():
    """A handle of its own: no other test of this module meets an option this one left behind."""
    return _capi.DeviceTree(*synth.balanced_tree(4))


def _set(lib, dev, name, value):
    rc = lib.st_tree_set_option(dev.handle, name.encode(), value)
    return rc, _capi.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RULES))
def test_option_rule(lib, optioned, name):
    accepted, refused, message = RULES[name]
    try:
        for value in accepted:
            assert _set(lib, optioned, name, value)[0] == _capi.ST_OK, (name, value)
        for value in refused:
            assert _set(lib, optioned, name, value) == (_capi.ST_ERR_ARG, message), (name, value)
    finally:
        assert _set(lib, optioned, name, DEFAULT[name])[0] == _capi.ST_OK


@pytest.mark.gpu
def test_reserve_cus_is_bounded_by_the_device(lib, optioned):
    cus = optioned.info().get("n_cu_device", 100000)      # (the device's count where info() reports it)
    message = "reserve_cus must be in [0, CUs of the device)"
    try:
        for value in (0, 1) + ((cus - 1,) if cus != 100000 else ()):
            assert _set(lib, optioned, "reserve_cus", value)[0] == _capi.ST_OK, value
        for value in (-1, cus):
            assert _set(lib, optioned, "reserve_cus", value) == (_capi.ST_ERR_ARG, message), value
    finally:
        assert _set(lib, optioned, "reserve_cus", 0)[0] == _capi.ST_OK


@pytest.mark.gpu
def test_info_follows_the_options_it_reports(lib, optioned):
    def info_after(name, value):
        assert _set(lib, optioned, name, value)[0] == _capi.ST_OK
        return optioned.info()

    try:
        # a tree of 31 nodes: ids fit 24 bits, so the wire formats are the options'
        assert info_after("wire48", 0)["host_wire_bytes_in"] == 8 and info_after("wire48", 1)["host_wire_bytes_in"] == 6
        assert info_after("wire24", 0)["host_wire_bytes_out"] == 8 and info_after("wire24", 1)["host_wire_bytes_out"] == 7
        # 2 and 0 hold whatever the tree; 1 leaves it to the tree's tables and size
        assert info_after("stream_hint", 2)["stream_hint"] == 1 and info_after("stream_hint", 0)["stream_hint"] == 0
        i = info_after("heap_lines", 0)
        assert i["heap_lines"] == 0 and i["heap_codes"] == 0
        # an explicit ladder_sums holds for every batch size: the bound goes, and 0 is reported as 0
        for value in (1, 0):
            i = info_after("ladder_sums", value)
            assert i["ladder_sums_max_pairs"] == 0 and i["ladder_sums"] in (0, value)
        assert optioned.info()["ladder_sums"] == 0
    finally:
        for name in ("wire48", "wire24", "stream_hint", "heap_lines", "ladder_sums"):
            assert _set(lib, optioned, name, DEFAULT[name])[0] == _capi.ST_OK
