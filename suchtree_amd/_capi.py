"""ctypes binding of libsuchtree_hip.so (the C ABI in include/suchtree_hip.h).

Loading fails loudly (``HipBackendError``) when the library has not been built:
there is no CPU fallback anywhere in this package.
"""
import ctypes
import math
import os
import threading

import numpy as np

from .exceptions import HipBackendError, InvalidNodeError, TreeStructureError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsuchtree_hip.so")

ST_OK, ST_ERR_ARG, ST_ERR_HIP, ST_ERR_BOUNDS, ST_ERR_NOMEM, ST_ERR_TREE, ST_ERR_MEASURE_ONLY = 0, 1, 2, 3, 4, 5, 6
STRATEGY = {"auto": 0, "walk": 1, "canopy": 2}
STRATEGY_NAME = {v: k for k, v in STRATEGY.items()}
BIG_BATCH_KERNEL = {0: "walk", 1: "canopy", 3: "canopy_sorted", 4: "walk_sorted", 5: "canopy_ladder"}      # ST_KERNEL_*

# ST_TABLE_* bits of st_tree_info.dropped_tables, in the order a table budget drops them
DROPPED_TABLES = ((1, "lineage_len"), (2, "lineage_sum"), (4, "tree_rmq"), (8, "rec_i"), (16, "rec_a4"), (32, "ranks"), (64, "canopy"))


def dropped_table_names(bits):
    return [name for bit, name in DROPPED_TABLES if bits & bit]


class TreeOptions(ctypes.Structure):
    """st_tree_options (include/suchtree_hip.h)."""
    _fields_ = [("table_budget_bytes", ctypes.c_int64), ("reserved", ctypes.c_int64 * 7)]


API_VERSION = 7      # include/suchtree_hip.h: ST_API_VERSION

# every symbol include/suchtree_hip.h declares (tests check the .so exports them all)
SYMBOLS = (
    "st_api_version", "st_tree_info_get_sized", "st_last_error", "st_device_count", "st_tree_create", "st_tree_create_multi", "st_tree_create_ex", "st_host_table_plan", "st_tree_devices",
    "st_host_chunk_plan", "st_host_chunk_owner", "st_tree_destroy", "st_tree_info_get",
    "st_distances_host", "st_distances_host_i32", "st_distances_device", "st_distances_device_f32", "st_distances_device_wire", "st_unpack_mrca24_device", "st_fault_check", "st_probe_last_choice", "st_tree_set_strategy",
    "st_tree_set_option", "st_triangle_device", "st_triangle_host", "st_grid_host", "st_knn_host",
    "st_quartets_host", "st_graph_matrices_host", "st_newick_open", "st_newick_fill", "st_newick_close",
    "st_host_depths", "st_link_sample_pairs", "st_bucket_moments", "st_device_malloc", "st_device_free", "st_memcpy_h2d", "st_memcpy_d2h",
    "st_device_synchronize", "st_compare_triangle_host", "st_compare_pairs_host", "st_clade_plan", "st_compare_clades_host",
    "st_compare_rows_host", "st_compare_triangle_ranks_host", "st_compare_pairs_ranks_host", "st_spearman_host",
    "st_quartet_positions", "st_compare_quartets_leaves_host", "st_compare_quartets_host",
    "st_compare_triangle_kendall_host", "st_compare_pairs_kendall_host", "st_kendall_arrays_host", "st_kendall_host",
    "st_hommola_permutation", "st_hommola_clades_host", "st_partner_dispersion_host", "st_dispersion_matrix",
    "st_unifrac_host", "st_unifrac_depths", "st_unifrac_quantise", "st_clade_ranges", "st_clade_match",
    "st_beta_dispersion_host", "st_beta_dispersion_matrix", "st_unifrac_null_host", "st_unifrac_null_depths",
    "st_mantel_codes", "st_mantel_quantise", "st_group_sums_codes", "st_parafit_codes", "st_class_sums_codes",
    "st_swap_null_tables", "st_swap_null_schedule", "st_dispersion_matrix_swap", "st_partner_dispersion_swap_host",
    "st_linkage_codes", "st_rf_tasks",
)

CLADE_RECT, CLADE_TRI = 0, 1     # include/suchtree_hip.h: ST_CLADE_RECT / ST_CLADE_TRI
CLADE_TILE = 8192                # ST_CLADE_TILE: pairs per tile of the clade reduction
KENDALL_TILE = 2048              # ST_KENDALL_TILE: keys per tile of the Kendall sort (a workgroup's share of a merge level)

# st_clade_segment as a numpy record
CLADE_SEGMENT = np.dtype([("first_pair", np.int64), ("n_pairs", np.int64), ("kind", np.int32), ("node", np.int32),
                          ("row_begin", np.int32), ("row_end", np.int32), ("col_begin", np.int32), ("col_end", np.int32)])


class PairMoments(ctypes.Structure):
    """st_pair_moments (include/suchtree_hip.h): sums about the shift (shift_x, shift_y) of the compare path."""
    _fields_ = [("n", ctypes.c_int64)] + [(k, ctypes.c_double) for k in
                                          "shift_x shift_y sx sy sxx syy sxy min_x max_x min_y max_y".split()]

    def as_dict(self):
        return {k: (int(getattr(self, k)) if k == "n" else float(getattr(self, k))) for k, _ in self._fields_}


# st_pair_moments as a numpy record (arrays of them: st_compare_clades_host, st_compare_rows_host)
PAIR_MOMENTS = np.dtype([("n", np.int64)] + [(k, np.float64) for k in
                                            "shift_x shift_y sx sy sxx syy sxy min_x max_x min_y max_y".split()])
assert PAIR_MOMENTS.itemsize == ctypes.sizeof(PairMoments)


class RankSums(ctypes.Structure):
    """st_rank_sums (include/suchtree_hip.h): the exact integer sums of Spearman's rank correlation."""
    _fields_ = [("n", ctypes.c_int64), ("n_nan", ctypes.c_int64), ("distinct_x", ctypes.c_int64), ("distinct_y", ctypes.c_int64),
                ("sxy_lo", ctypes.c_uint64), ("sxy_hi", ctypes.c_int64), ("sxx_lo", ctypes.c_uint64), ("sxx_hi", ctypes.c_uint64),
                ("syy_lo", ctypes.c_uint64), ("syy_hi", ctypes.c_uint64)]

    @property
    def sxy(self):
        return (int(self.sxy_hi) << 64) + int(self.sxy_lo)

    @property
    def sxx(self):
        return (int(self.sxx_hi) << 64) + int(self.sxx_lo)

    @property
    def syy(self):
        return (int(self.syy_hi) << 64) + int(self.syy_lo)


class KendallCounts(ctypes.Structure):
    """st_kendall_counts (include/suchtree_hip.h): the exact integer counts of Kendall's tau-b."""
    _fields_ = [("n", ctypes.c_int64), ("n_nan", ctypes.c_int64), ("discordant", ctypes.c_uint64), ("ties_x", ctypes.c_uint64),
                ("ties_y", ctypes.c_uint64), ("ties_xy", ctypes.c_uint64)]

    @property
    def concordant(self):
        """n0 - ties_x - ties_y + ties_xy - discordant, n0 = n (n - 1) / 2; 0 when a pair held a NaN."""
        n = int(self.n)
        if self.n_nan > 0 or n < 2:
            return 0
        return n * (n - 1) // 2 - int(self.ties_x) - int(self.ties_y) + int(self.ties_xy) - int(self.discordant)

    def as_tuple(self):
        return tuple(int(getattr(self, k)) for k, _ in self._fields_)


HOMMOLA_MAX_UNIVERSE = 16384     # ST_HOMMOLA_MAX_UNIVERSE: leaves per universe of st_hommola_clades_host
# st_hommola_clade as a numpy record
HOMMOLA_CLADE = np.dtype([("node", np.int32), ("leaf_begin", np.int32), ("leaf_count", np.int32), ("link_begin", np.int32),
                          ("link_count", np.int32), ("reserved", np.int32)])


def hommola_permutation(seed, node, p, side, n, device=-1):
    """st_hommola_permutation: the int32 permutation of (seed, clade node, permutation index p, side, universe size n) that
    st_hommola_clades_host applies; ``device`` -1 = computed on the host (no GPU), else by the sort of the relabelling kernel."""
    n = int(n)
    out = np.empty(max(n, 0), dtype=np.int32)
    check(load().st_hommola_permutation(int(device), int(seed) & 0xFFFFFFFFFFFFFFFF, int(node), int(p), int(side), n, _ptr(out) if n > 0 else None))
    return out


# st_dispersion_record as a numpy record
DISPERSION_RECORD = np.dtype([("pair_sum", np.float64), ("nearest_sum", np.float64)])


def _dispersion_sets(sets, n_univ):
    """(set_pos int32, offsets int64, n_sets) of an iterable of position collections, or of a (set_pos, offsets) tuple of
    arrays; ValueError for a position outside the universe or a set that is not strictly increasing (the library checks
    again)."""
    if isinstance(sets, tuple) and len(sets) == 2 and all(isinstance(a, np.ndarray) for a in sets):
        pos = np.ascontiguousarray(sets[0], dtype=np.int32)
        off = np.ascontiguousarray(sets[1], dtype=np.int64)
        if pos.ndim != 1 or off.ndim != 1 or len(off) < 1:
            raise ValueError("set_pos must be 1-D and offsets hold n_sets + 1 entries")
        return pos, off, len(off) - 1
    rows = [np.asarray(r, dtype=np.int64).ravel() for r in sets]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([len(r) for r in rows], out=off[1:])
    pos = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    if len(pos) and (pos.min() < 0 or pos.max() >= n_univ):
        raise ValueError("a position outside the universe of %d" % n_univ)
    return pos.astype(np.int32), off, len(rows)


def _dispersion_args(permutations, stream, chunk_tasks):
    if int(permutations) < 0:
        raise ValueError("permutations < 0")
    if int(stream) < 0 or int(stream) > 0x7FFFFFFF:
        raise ValueError("stream must be a non-negative int32")
    if int(chunk_tasks) < 0:
        raise ValueError("chunk_tasks < 0")


def _square_matrix(D):
    """(D as a C-order float32 array, n) of an (n, n) matrix"""
    D = np.ascontiguousarray(D, dtype=np.float32)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError("D must be a square matrix")
    return D, int(D.shape[0])


def dispersion_matrix(D, sets, permutations, seed, stream=0, device=-1, chunk_tasks=0):
    """st_dispersion_matrix: the (n_sets, permutations + 1) array of DISPERSION_RECORD of the position sets ``sets`` (an
    iterable of strictly increasing position collections, or a (set_pos, offsets) tuple of arrays) over the C-order
    float32 (n, n) matrix ``D``; ``device`` -1 = the host restatement (no GPU), else the kernels on that device."""
    D, n = _square_matrix(D)
    _dispersion_args(permutations, stream, chunk_tasks)
    pos, off, n_sets = _dispersion_sets(sets, n)
    out = np.zeros((n_sets, int(permutations) + 1), dtype=DISPERSION_RECORD)
    check(load().st_dispersion_matrix(int(device), _ptr(D), n, _arg(pos), len(pos), _ptr(off), n_sets, int(permutations),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(chunk_tasks), _arg(out)))
    return out


def swap_iterations(iterations, n_links):
    """The trials of a swap chain: ``iterations``, or for None the library's default max(1000, 10 x the links)."""
    if iterations is None:
        return max(1000, 10 * int(n_links))
    if int(iterations) < 0:
        raise ValueError("iterations < 0")
    return int(iterations)


def _swap_links(off):
    return int(off[-1] - off[0])


def swap_null_tables(sets, n_univ, permutations=0, begin=0, iterations=None, seed=0, stream=0, device=-1):
    """st_swap_null_tables: (tables, offsets, accepted) of the degree-preserving swap null over the position sets ``sets`` (as
    in ``dispersion_matrix``; a row per set, a column per position of the universe of ``n_univ``).  ``tables`` is the
    (permutations + 1, n_pos) uint16 array of table rows begin .. begin + permutations -- row p holds the randomised sets
    of chain p, sorted, at the offsets ``offsets`` of the observed ones; p = 0 is the observation -- and ``accepted`` the
    swaps each chain made of its ``iterations`` trials (None: max(1000, 10 x the links)).  ``device`` -1 = the host
    restatement (no GPU), else k_swap_chains on that device: the same values."""
    n_univ = int(n_univ)
    _dispersion_args(permutations, stream, 0)
    if int(begin) < 0:
        raise ValueError("begin < 0")
    pos, off, n_sets = _dispersion_sets(sets, n_univ)
    rows = int(permutations) + 1
    tables = np.zeros((rows, len(pos)), dtype=np.uint16)
    accepted = np.zeros(rows, dtype=np.int64)
    check(load().st_swap_null_tables(int(device), n_univ, _arg(pos), len(pos), _ptr(off), n_sets, int(begin), rows,
                                     swap_iterations(iterations, _swap_links(off)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream),
                                     _arg(tables), _arg(accepted)))
    return tables, off, accepted


def swap_null_schedule(sets, n_univ, p, iterations=None, seed=0, stream=0):
    """st_swap_null_schedule: (table row, accepted, steps) of chain ``p`` run on the host in the schedule of the device's
    wave -- batches of 64 trials cut at the first lane that shares a row with an earlier one; ``steps`` batches for
    ``iterations`` trials.  The row and ``accepted`` are those of ``swap_null_tables``."""
    n_univ = int(n_univ)
    _dispersion_args(0, stream, 0)
    pos, off, n_sets = _dispersion_sets(sets, n_univ)
    row = np.zeros(len(pos), dtype=np.uint16)
    accepted, steps = ctypes.c_int64(0), ctypes.c_int64(0)
    check(load().st_swap_null_schedule(n_univ, _arg(pos), len(pos), _ptr(off), n_sets, int(p), swap_iterations(iterations, _swap_links(off)),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), _arg(row), ctypes.byref(accepted), ctypes.byref(steps)))
    return row, int(accepted.value), int(steps.value)


def dispersion_matrix_swap(D, sets, permutations, seed, iterations=None, stream=0, device=-1, chunk_tasks=0):
    """st_dispersion_matrix_swap: (records, accepted) -- the (n_sets, permutations + 1) array of DISPERSION_RECORD of
    ``dispersion_matrix`` under the swap null (record (r, p) over set r of table row p of ``swap_null_tables``) and the
    accepted swaps of every chain."""
    D, n = _square_matrix(D)
    _dispersion_args(permutations, stream, chunk_tasks)
    pos, off, n_sets = _dispersion_sets(sets, n)
    out = np.zeros((n_sets, int(permutations) + 1), dtype=DISPERSION_RECORD)
    accepted = np.zeros(int(permutations) + 1, dtype=np.int64)
    check(load().st_dispersion_matrix_swap(int(device), _ptr(D), n, _arg(pos), len(pos), _ptr(off), n_sets, int(permutations),
                                           swap_iterations(iterations, _swap_links(off)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream),
                                           int(chunk_tasks), _arg(out), _arg(accepted)))
    return out, accepted


UNIFRAC_MAX_UNIVERSE = 1 << 20     # ST_UNIFRAC_MAX_UNIVERSE: leaves per universe of st_unifrac_host
UNIFRAC_LANE_MAX = 512             # ST_UNIFRAC_LANE_MAX: pairs of |A| + |B| up to this are merged by one lane, larger ones by one wave


def _unifrac_range(n_sets, begin, count, chunk_pairs):
    """(begin, count) of a triangle range over ``n_sets`` sets, ``count`` None = up to the last pair."""
    total = n_sets * (n_sets - 1) // 2
    begin = int(begin)
    count = total - begin if count is None else int(count)
    if begin < 0 or count < 0 or begin + count > total:
        raise ValueError("pairs [%d, +%d) of a triangle of %d" % (begin, count, total))
    if int(chunk_pairs) < 0:
        raise ValueError("chunk_pairs < 0")
    return begin, count


def _quantised_depths(d_q, h_q):
    """(d_q, h_q) as C-order int64 arrays of n depths and n - 1"""
    d_q = np.ascontiguousarray(d_q, dtype=np.int64)
    h_q = np.ascontiguousarray(h_q, dtype=np.int64)
    if d_q.ndim != 1 or h_q.ndim != 1 or len(h_q) != max(len(d_q) - 1, 0):
        raise ValueError("d_q must hold n depths and h_q n - 1")
    return d_q, h_q


def beta_dispersion_matrix(D, sets, begin=0, count=None, exclude_shared=False, permutations=0, seed=0, stream=0, device=-1, chunk_tasks=0):
    """st_beta_dispersion_matrix: the (count, 2, permutations + 1) array of DISPERSION_RECORD (``pair_sum`` holds the cross
    sum) of pairs [begin, begin + count) of the triangle over the position sets ``sets`` (as in ``dispersion_matrix``),
    directions i -> j and j -> i, over the C-order float32 (n, n) matrix ``D``; ``device`` -1 = the host restatement (no
    GPU), else the kernels on that device."""
    D, n = _square_matrix(D)
    _dispersion_args(permutations, stream, chunk_tasks)
    pos, off, n_sets = _dispersion_sets(sets, n)
    begin, count = _unifrac_range(n_sets, begin, count, 0)
    out = np.zeros((count, 2, int(permutations) + 1), dtype=DISPERSION_RECORD)
    check(load().st_beta_dispersion_matrix(int(device), _ptr(D), n, _arg(pos), len(pos), _ptr(off), n_sets, begin, count, int(bool(exclude_shared)),
                                           int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(chunk_tasks), _arg(out)))
    return out


def unifrac_quantise(d, h, shift=None):
    """st_unifrac_quantise: (d_q int64, h_q int64, shift used) of the float32 depths ``d`` (n) and ``h`` (n - 1) under the
    fixed-point rule of st_unifrac_host; ``shift`` None = automatic.  ValueError for a depth that is not finite or a shift
    that puts a value at 2^40 or more."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    if d.ndim != 1 or h.ndim != 1 or len(h) != max(len(d) - 1, 0):
        raise ValueError("d must hold n depths and h n - 1")
    d_q, h_q = np.zeros(len(d), dtype=np.int64), np.zeros(len(h), dtype=np.int64)
    used = ctypes.c_int32(0)
    check(load().st_unifrac_quantise(_arg(d), _arg(h), len(d), -1 if shift is None else int(shift), _arg(d_q), _arg(h_q), ctypes.byref(used)))
    return d_q, h_q, int(used.value)


def unifrac_depths(d_q, h_q, sets, begin=0, count=None, device=-1, chunk_pairs=0):
    """st_unifrac_depths: (pd_q, union_q), the int64 PD of every set and union sum of pairs [begin, begin + count) of the
    triangle over the position sets ``sets`` (as in ``dispersion_matrix``), from the quantised depths ``d_q`` (n) and
    ``h_q`` (n - 1); ``device`` -1 = the host restatement (no GPU), else the kernels on that device."""
    d_q, h_q = _quantised_depths(d_q, h_q)
    pos, off, n_sets = _dispersion_sets(sets, len(d_q))
    begin, count = _unifrac_range(n_sets, begin, count, chunk_pairs)
    pd_q, union_q = np.zeros(n_sets, dtype=np.int64), np.zeros(count, dtype=np.int64)
    check(load().st_unifrac_depths(int(device), _arg(d_q), _arg(h_q), len(d_q), _arg(pos), len(pos), _ptr(off), n_sets, begin, count,
                                   int(chunk_pairs), _arg(pd_q), _arg(union_q)))
    return pd_q, union_q


def unifrac_null_depths(d_q, h_q, sets, begin=0, count=None, permutations=0, seed=0, stream=0, device=-1, chunk_tasks=0, pd=True, union=True):
    """st_unifrac_null_depths: (pd_q (n_sets, permutations + 1), union_q (count, permutations + 1)), the int64 PD of every
    set and union sum of pairs [begin, begin + count) of the triangle over the position sets ``sets`` (as in
    ``dispersion_matrix``) under every permutation p of the taxa-labels null, from the quantised depths ``d_q`` (n) and
    ``h_q`` (n - 1); column 0 is ``unifrac_depths``.  ``device`` -1 = the host restatement (no GPU), else the kernels on
    that device.  ``pd`` / ``union`` False: that output is not computed and comes back as None."""
    d_q, h_q = _quantised_depths(d_q, h_q)
    _dispersion_args(permutations, stream, chunk_tasks)
    pos, off, n_sets = _dispersion_sets(sets, len(d_q))
    begin, count = _unifrac_range(n_sets, begin, count, 0)
    R = int(permutations) + 1
    pd_q = np.zeros((n_sets, R), dtype=np.int64) if pd else None
    union_q = np.zeros((count, R), dtype=np.int64) if union else None
    check(load().st_unifrac_null_depths(int(device), _arg(d_q), _arg(h_q), len(d_q), _arg(pos), len(pos), _ptr(off), n_sets, begin, count,
                                        int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(chunk_tasks),
                                        _ptr(pd_q) if pd else None, _ptr(union_q) if union else None))
    return pd_q, union_q


MANTEL_SHIFT_AUTO = -2147483648     # ST_MANTEL_SHIFT_AUTO
# st_mantel_sums as a numpy record
MANTEL_SUMS = np.dtype([("sxy_lo", np.uint64), ("sxy_hi", np.int64), ("sxz_lo", np.uint64), ("sxz_hi", np.int64)])
MANTEL_MOMENT_NAMES = ("sx", "sy", "sz", "sxx", "syy", "szz", "syz")


class MantelMoments(ctypes.Structure):
    """st_mantel_moments (include/suchtree_hip.h): the sums of the Mantel test that no permutation changes, as lo / hi pairs."""
    _fields_ = [f for k in MANTEL_MOMENT_NAMES for f in ((k + "_lo", ctypes.c_uint64), (k + "_hi", ctypes.c_int64))]

    def as_dict(self):
        return {k: (int(getattr(self, k + "_hi")) << 64) + int(getattr(self, k + "_lo")) for k in MANTEL_MOMENT_NAMES}


def mantel_ints(records, name):
    """The 128-bit sums ``name`` ("sxy" / "sxz") of an array of MANTEL_SUMS as a list of Python ints."""
    lo, hi = records[name + "_lo"].tolist(), records[name + "_hi"].tolist()
    return [(h << 64) + l for l, h in zip(lo, hi)]


def mantel_codes(x_sq, y, z=None, permutations=0, seed=0, stream=0, device=-1, chunk_tasks=0):
    """st_mantel_codes: (moments dict of Python ints, records) of the square int32 matrix ``x_sq`` (n, n) against the
    condensed int32 ``y`` and, for the partial test, ``z`` (n (n - 1) / 2 each, pair (i, j) at i (i - 1) / 2 + j): the
    permutations + 1 records of MANTEL_SUMS, record 0 the observation.  ``device`` -1 = the host restatement (no GPU),
    else the kernels on that device."""
    x_sq = np.ascontiguousarray(x_sq, dtype=np.int32)
    if x_sq.ndim != 2 or x_sq.shape[0] != x_sq.shape[1]:
        raise ValueError("x_sq must be a square matrix")
    n = int(x_sq.shape[0])
    m = n * (n - 1) // 2
    y = np.ascontiguousarray(y, dtype=np.int32)
    z = None if z is None else np.ascontiguousarray(z, dtype=np.int32)
    for name, v in (("y", y), ("z", z)):
        if v is not None and (v.ndim != 1 or len(v) != m):
            raise ValueError("%s must hold the %d pairs of %d objects" % (name, m, n))
    _dispersion_args(permutations, stream, chunk_tasks)
    out = np.zeros(int(permutations) + 1, dtype=MANTEL_SUMS)
    moments = MantelMoments()
    check(load().st_mantel_codes(int(device), _ptr(x_sq), _arg(y), None if z is None else _arg(z), n, int(permutations),
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(chunk_tasks), ctypes.byref(moments), _ptr(out)))
    return moments.as_dict(), out


def mantel_quantise(v, shift=None):
    """st_mantel_quantise: (int32 codes llrint(ldexp(v, shift)) in the shape of ``v``, shift used); ``shift`` None = the
    one that puts the largest |code| in [2^30, 2^31).  ValueError for a NaN or an infinity (naming its index in C order)
    or a shift that puts a code at 2^31 or more."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.int32)
    used = ctypes.c_int32(0)
    check(load().st_mantel_quantise(_arg(v), v.size, MANTEL_SHIFT_AUTO if shift is None else int(shift), _arg(out), ctypes.byref(used)))
    return out, int(used.value)


GROUP_MAX = 256     # ST_GROUP_MAX: labels of st_group_sums_codes are bytes


def group_sums_codes(y, group, n_groups, permutations, seed=0, stream=0, device=-1, chunk_tasks=0):
    """st_group_sums_codes: the int64 (permutations + 1, n_groups) sums of the condensed int32 codes ``y`` (n (n - 1) / 2,
    pair (i, j) at i (i - 1) / 2 + j) over the pairs whose two objects carry label h under permutation p of the labels
    ``group`` (n values below ``n_groups`` <= GROUP_MAX); row 0 is the observation.  ``device`` -1 = the host restatement
    (no GPU), else the kernels on that device."""
    g = np.asarray(group)
    if g.ndim != 1:
        raise ValueError("group must hold one label per object")
    n = len(g)
    if n and (g.min() < 0 or g.max() >= GROUP_MAX):
        i = int(np.flatnonzero((g < 0) | (g >= GROUP_MAX))[0])
        raise ValueError("group[%d] = %d: labels are 0 to %d" % (i, int(g[i]), GROUP_MAX - 1))
    g = np.ascontiguousarray(g, dtype=np.uint8)
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.ndim != 1 or len(y) != n * (n - 1) // 2:
        raise ValueError("y must hold the %d pairs of %d objects" % (n * (n - 1) // 2, n))
    _dispersion_args(permutations, stream, chunk_tasks)
    n_groups = int(n_groups)
    out = np.zeros((int(permutations) + 1, max(min(n_groups, GROUP_MAX), 0)), dtype=np.int64)
    check(load().st_group_sums_codes(int(device), _arg(y), n, _arg(g), n_groups, int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(stream), int(chunk_tasks), _ptr(out) if out.size else None))
    return out


CLASS_MAX = 64       # ST_CLASS_MAX: classes per call of st_class_sums_codes
CLASS_NONE = 255     # ST_CLASS_NONE: a pair that is in no class


def class_sums_codes(y, cls, n_classes, permutations, seed=0, stream=0, device=-1, chunk_tasks=0):
    """st_class_sums_codes: the int64 (permutations + 1, n_classes) sums of the condensed int32 codes ``y`` (n (n - 1) / 2,
    pair (i, j) at i (i - 1) / 2 + j) filed under the class of the relabelled pair: ``cls`` holds, condensed in the same
    order, the class of each pair (below ``n_classes`` <= CLASS_MAX) or CLASS_NONE; row 0 is the observation.  ``device``
    -1 = the host restatement (no GPU), else the kernels on that device."""
    c = np.asarray(cls)
    y = np.ascontiguousarray(y, dtype=np.int32)
    if y.ndim != 1 or c.ndim != 1 or len(c) != len(y):
        raise ValueError("y and cls must be condensed and of one length")
    m = len(y)
    n = (1 + math.isqrt(8 * m + 1)) // 2
    if n * (n - 1) // 2 != m:
        raise ValueError("%d pairs are not the triangle of a square matrix" % m)
    if m and (c.min() < 0 or c.max() > CLASS_NONE):
        k = int(np.flatnonzero((c < 0) | (c > CLASS_NONE))[0])
        raise ValueError("cls[%d] = %d: classes are bytes" % (k, int(c[k])))
    c = np.ascontiguousarray(c, dtype=np.uint8)
    _dispersion_args(permutations, stream, chunk_tasks)
    n_classes = int(n_classes)
    out = np.zeros((int(permutations) + 1, max(min(n_classes, CLASS_MAX), 0)), dtype=np.int64)
    check(load().st_class_sums_codes(int(device), _arg(y), _arg(c), n, n_classes, int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(stream), int(chunk_tasks), _ptr(out) if out.size else None))
    return out


# st_parafit_sum as a numpy record
PARAFIT_SUM = np.dtype([("lo", np.uint64), ("hi", np.int64)])


def parafit_ints(records):
    """The 128-bit sums of an array of PARAFIT_SUM as a (nested) list of Python ints, in the array's shape."""
    lo, hi = records["lo"].ravel().tolist(), records["hi"].ravel().tolist()
    flat = [(h << 64) + l for l, h in zip(lo, hi)]
    if records.ndim == 2:
        w = records.shape[1]
        return [flat[r * w:(r + 1) * w] for r in range(records.shape[0])]
    return flat


def parafit_codes(g_f, g_s, link_f, link_s, stream_f, permutations=0, seed=0, device=-1, chunk_tasks=0, keep=False):
    """st_parafit_codes: (total, link_obs, link_n_ge, link_all) of the square int32 code matrices ``g_f`` (n_f, n_f) and
    ``g_s`` (n_s, n_s), the links (``link_f[l]``, ``link_s[l]``) as positions, strictly increasing in (f, s) order, and
    one stream id per F position: ``total`` the permutations + 1 records of PARAFIT_SUM, ``link_obs`` one per link,
    ``link_n_ge`` int64 per link and, with ``keep``, ``link_all`` of shape (permutations + 1, L), else None.  ``device``
    -1 = the host restatement (no GPU), else the kernels on that device."""
    g_f = np.ascontiguousarray(g_f, dtype=np.int32)
    g_s = np.ascontiguousarray(g_s, dtype=np.int32)
    for name, g in (("g_f", g_f), ("g_s", g_s)):
        if g.ndim != 2 or g.shape[0] != g.shape[1]:
            raise ValueError("%s must be a square matrix" % name)
    link_f = np.ascontiguousarray(link_f, dtype=np.int32)
    link_s = np.ascontiguousarray(link_s, dtype=np.int32)
    stream_f = np.ascontiguousarray(stream_f, dtype=np.int32)
    if link_f.ndim != 1 or link_s.shape != link_f.shape:
        raise ValueError("link_f and link_s must be 1-D and of one length")
    if stream_f.shape != (g_f.shape[0],):
        raise ValueError("stream_f must hold one stream id per F position")
    _dispersion_args(permutations, 0, chunk_tasks)
    L, R = len(link_f), int(permutations) + 1
    total = np.zeros(R, dtype=PARAFIT_SUM)
    link_obs = np.zeros(L, dtype=PARAFIT_SUM)
    link_n_ge = np.zeros(L, dtype=np.int64)
    link_all = np.zeros((R, L), dtype=PARAFIT_SUM) if keep else None
    check(load().st_parafit_codes(int(device), _ptr(g_f), int(g_f.shape[0]), _ptr(g_s), int(g_s.shape[0]), _arg(link_f), _arg(link_s), L,
                                  _arg(stream_f), int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunk_tasks), _ptr(total), _arg(link_obs),
                                  _arg(link_n_ge), _ptr(link_all) if keep else None))
    return total, link_obs, link_n_ge, link_all


CLADE_MATCH_MAX_LEAVES = 1 << 18    # ST_CLADE_MATCH_MAX_LEAVES: leaves per list of st_clade_ranges / st_clade_match


def clade_ranges(parent, leaf_ids, rooted=False):
    """st_clade_ranges (host only): (order, node, lo, hi) of one tree over the listed leaves -- ``order[k]`` is the index in
    ``leaf_ids`` of the leaf at depth-first position k, and the eligible induced clades are the nodes ``node`` with the
    position ranges [lo, hi), in ``get_internal_nodes()`` order.  InvalidNodeError for an id outside the tree, ValueError
    for one that is not a leaf or is listed twice and for fewer than 4 or more than CLADE_MATCH_MAX_LEAVES leaves."""
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    leaf_ids = np.ascontiguousarray(leaf_ids, dtype=np.int64)
    if parent.ndim != 1 or leaf_ids.ndim != 1:
        raise ValueError("parent and leaf_ids must be 1-D")
    m = len(leaf_ids)
    if m > CLADE_MATCH_MAX_LEAVES:      # (before the outputs are sized)
        raise ValueError("a list of %d leaves: at most %d" % (m, CLADE_MATCH_MAX_LEAVES))
    order = np.zeros(m, dtype=np.int32)
    node, lo, hi = (np.zeros(max(m - 1, 1), dtype=np.int32) for _ in range(3))
    n, bad = ctypes.c_int32(0), ctypes.c_int64(-1)
    rc = load().st_clade_ranges(_arg(parent), len(parent), _arg(leaf_ids), m, 1 if rooted else 0, _ptr(order), _ptr(node), _ptr(lo), _ptr(hi),
                                ctypes.byref(n), ctypes.byref(bad))
    check(rc, len(parent), bad.value)
    k = int(n.value)
    return order, node[:k].copy(), lo[:k].copy(), hi[:k].copy()


def clade_match(m, pos_b, a_lo, a_hi, b_lo, b_hi, rooted=False, device=-1, chunk_rows=0):
    """st_clade_match: (distance, match, intersection), one int32 each per row [a_lo, a_hi) of tree A: the least delta over
    the candidates [b_lo, b_hi) of tree B, the index of the candidate that has it (the lowest on a tie) and the leaves
    the two share; -1, -1, 0 without candidates.  ``pos_b[k]`` is B's position of the leaf at A's position k.  ``device``
    -1 = the host restatement (no GPU), else the kernel on that device: the same integers."""
    arr = lambda a: np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    pos_b, a_lo, a_hi, b_lo, b_hi = arr(pos_b), arr(a_lo), arr(a_hi), arr(b_lo), arr(b_hi)
    if any(v.ndim != 1 for v in (pos_b, a_lo, a_hi, b_lo, b_hi)) or len(pos_b) != int(m) or len(a_lo) != len(a_hi) or len(b_lo) != len(b_hi):
        raise ValueError("pos_b must hold m positions, and lo and hi of a list the same number of ranges")
    if int(chunk_rows) < 0:
        raise ValueError("chunk_rows < 0")
    n_a = len(a_lo)
    out = [np.zeros(n_a, dtype=np.int32) for _ in range(3)]
    check(load().st_clade_match(int(device), int(m), _arg(pos_b), _arg(a_lo), _arg(a_hi), n_a, _arg(b_lo), _arg(b_hi), len(b_lo),
                                0 if rooted else 1, int(chunk_rows), _arg(out[0]), _arg(out[1]), _arg(out[2])))
    return tuple(out)


LINKAGE_METHODS = {"average": 0, "single": 1, "complete": 2}      # include/suchtree_hip.h: ST_LINKAGE_AVERAGE / _SINGLE / _COMPLETE
LINKAGE_MAX_OBJECTS = 16384      # ST_LINKAGE_MAX_OBJECTS
LINKAGE_MAX_WEIGHT = 65536       # ST_LINKAGE_MAX_WEIGHT: the total of the weights
# st_linkage_row as a numpy record
LINKAGE_ROW = np.dtype([("num", np.int64), ("den", np.int64), ("left", np.int32), ("right", np.int32), ("size", np.int64)])


def linkage_codes(codes, weights=None, method="average", device=-1):
    """st_linkage_codes: the n - 1 records of LINKAGE_ROW of the exact agglomerative clustering of the condensed int32
    ``codes`` (n (n - 1) / 2 values >= 0, pair (i, j) at i (i - 1) / 2 + j) under ``method`` ("average" = UPGMA, "single",
    "complete"): row t merges the clusters ``left`` < ``right`` (ids below n are objects, n + s is the cluster of row s)
    at the value ``num`` / ``den`` into one of ``size`` objects; of the pairs of least value the one with the least
    slots is taken.  ``weights``: n int32 >= 1, object i stands for that many coincident objects.  ``device`` -1 = the
    host restatement (no GPU), else the kernels on that device: the same integers."""
    if method not in LINKAGE_METHODS:
        raise ValueError("method must be one of %s" % (tuple(LINKAGE_METHODS),))
    codes = np.asarray(codes)
    if codes.ndim != 1:
        raise ValueError("codes must be condensed")
    m = len(codes)
    n = (1 + math.isqrt(8 * m + 1)) // 2
    if n * (n - 1) // 2 != m:
        raise ValueError("%d pairs are not the triangle of a square matrix" % m)
    if n > LINKAGE_MAX_OBJECTS:      # (before the square is sized)
        raise ValueError("n = %d objects: 2 to %d" % (n, LINKAGE_MAX_OBJECTS))
    if m and (codes.min() < 0 or codes.max() > 0x7FFFFFFF):
        k = int(np.flatnonzero((codes < 0) | (codes > 0x7FFFFFFF))[0])
        raise ValueError("codes[%d] = %d %s" % (k, int(codes[k]), "is negative" if codes[k] < 0 else "does not fit int32"))
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    if weights is not None:
        weights = np.asarray(weights)
        if weights.shape != (n,):
            raise ValueError("weights must hold one value per object (%d)" % n)
        if n and (weights.min() < 1 or weights.max() > LINKAGE_MAX_WEIGHT):
            i = int(np.flatnonzero((weights < 1) | (weights > LINKAGE_MAX_WEIGHT))[0])
            raise ValueError("weights[%d] = %d: 1 to %d" % (i, int(weights[i]), LINKAGE_MAX_WEIGHT))
        weights = np.ascontiguousarray(weights, dtype=np.int32)
    out = np.zeros(max(n - 1, 0), dtype=LINKAGE_ROW)
    check(load().st_linkage_codes(int(device), _arg(codes), n, None if weights is None else _arg(weights), LINKAGE_METHODS[method],
                                  _ptr(out) if len(out) else None))
    return out


RF_MAX_LEAVES = 16384      # ST_RF_MAX_LEAVES: common leaves of st_rf_tasks


def rf_tasks(m, where, clade_offsets, lo, hi, rooted=False, align=None, task_i=None, task_j=None, task_p=None, begin=0, count=None,
             want_count=True, device=-1, chunk_tasks=0):
    """st_rf_tasks: (shared, counts).  ``where`` is (n_trees, m) int32 -- row t takes common leaf k to its depth-first
    position in tree t -- and tree t's clades are the ranges ``lo`` / ``hi`` at ``clade_offsets[t] : clade_offsets[t + 1]``
    (n_trees + 1 int64 offsets from 0).  Tasks: ``task_i`` / ``task_j`` (and ``task_p``: a row of ``align`` -- (n_align, m)
    int32 permutations -- or -1 for the identity), or without them the pairs [begin, begin + count) of the triangle
    k = i (i - 1) / 2 + j, j < i (``count=None``: to its end).  ``shared[t]`` (int32) is the number of clades of tree j
    that are clades of tree i under the task's alignment: common leaf k of i meets common leaf a[k] of j.  ``counts``
    (int64 per clade of the concatenated list, None with ``want_count=False``): every shared clade adds 1 to its own
    entry and 1 to its match's.  ``device`` -1 = the host restatement (no GPU), else the kernel on that device: the same
    integers.  ValueError for a bad argument, IndexError for a task that names a tree or an alignment out of range."""
    arr = lambda a: np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
    m = int(m)
    if m > RF_MAX_LEAVES:      # (before anything is sized by it)
        raise ValueError("a list of %d leaves: at most %d" % (m, RF_MAX_LEAVES))
    where, lo, hi = arr(where), arr(lo), arr(hi)
    offsets = np.ascontiguousarray(clade_offsets, dtype=np.int64)
    if where.ndim != 2 or where.shape[1] != m or offsets.ndim != 1 or len(offsets) != len(where) + 1 or lo.ndim != 1 or lo.shape != hi.shape:
        raise ValueError("where must be (n_trees, m), clade_offsets n_trees + 1 offsets, and lo and hi the same number of ranges")
    if len(lo) != int(offsets[-1]):
        raise ValueError("clade_offsets end at %d, lo and hi hold %d ranges" % (int(offsets[-1]), len(lo)))
    n_trees = len(where)
    if align is not None:
        align = arr(align)
        if align.ndim != 2 or align.shape[1] != m:
            raise ValueError("align must be (n_align, m)")
    if int(chunk_tasks) < 0:
        raise ValueError("chunk_tasks < 0")
    if task_i is None and task_j is None:
        if task_p is not None:
            raise ValueError("task_p without task_i and task_j")
        total = n_trees * (n_trees - 1) // 2
        begin = int(begin)
        n_tasks = max(total - begin, 0) if count is None else int(count)
    else:
        if task_i is None or task_j is None:
            raise ValueError("task_i and task_j come together")
        task_i, task_j = arr(task_i), arr(task_j)
        task_p = None if task_p is None else arr(task_p)
        if task_i.ndim != 1 or task_i.shape != task_j.shape or (task_p is not None and task_p.shape != task_i.shape):
            raise ValueError("the task arrays must be 1-D and of equal length")
        if int(begin) != 0 or (count is not None and int(count) != len(task_i)):
            raise ValueError("begin and count belong to the triangle form")
        begin, n_tasks = 0, len(task_i)
    shared = np.zeros(max(n_tasks, 0), dtype=np.int32)
    counts = np.zeros(len(lo), dtype=np.int64) if want_count else None
    opt = lambda a: None if a is None or not a.size else _arg(a)      # noqa: E731
    rc = load().st_rf_tasks(int(device), m, n_trees, opt(where), _arg(offsets), opt(lo), opt(hi), 0 if rooted else 1, opt(align),
                            0 if align is None else len(align), opt(task_i), opt(task_j), opt(task_p), n_tasks, begin, int(chunk_tasks),
                            opt(shared), opt(counts))
    if rc == ST_ERR_BOUNDS:
        raise IndexError(last_error())
    check(rc)
    return shared, counts


QUARTET_MODE = {"all": 0, "sample": 1}     # include/suchtree_hip.h: ST_QUARTET_ALL / ST_QUARTET_SAMPLE
QUARTET_MAX_LEAVES_ALL = 65536


class QuartetTable(ctypes.Structure):
    """st_quartet_table (include/suchtree_hip.h): cell[i][j] = quartets of class i in tree x and class j in tree y."""
    _fields_ = [("n", ctypes.c_int64), ("cell", (ctypes.c_int64 * 4) * 4)]

    def as_array(self):
        return np.array([[int(v) for v in row] for row in self.cell], dtype=np.int64)


def quartet_positions(mode, seed, m, k_begin, k_count, device=-1):
    """st_quartet_positions: the int32 (k_count, 4) positions of quartets [k_begin, k_begin + k_count) of ``mode``
    ("all" / "sample") among m leaves; ``device`` -1 = computed on the host (no GPU), else by the generator kernel."""
    if mode not in QUARTET_MODE:
        raise ValueError("mode must be 'all' or 'sample'")
    if int(k_count) < 0:
        raise ValueError("negative count")
    out = np.empty((int(k_count), 4), dtype=np.int32)
    check(load().st_quartet_positions(int(device), QUARTET_MODE[mode], int(seed) & 0xFFFFFFFFFFFFFFFF, int(m), int(k_begin),
                                      int(k_count), _ptr(out) if len(out) else None))
    return out


def spearman_host(x, y):
    """st_spearman_host: the exact rank sums (``RankSums``) of two float32 arrays of equal length, on the host."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D arrays of equal length")
    out = RankSums()
    check(load().st_spearman_host(_ptr(x) if len(x) else None, _ptr(y) if len(y) else None, len(x), ctypes.byref(out)))
    return out


def _float_columns(x, y):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D arrays of equal length")
    return x, y


def kendall_host(x, y):
    """st_kendall_host: the exact Kendall counts (``KendallCounts``) of two float32 arrays of equal length, on the host."""
    x, y = _float_columns(x, y)
    out = KendallCounts()
    check(load().st_kendall_host(_ptr(x) if len(x) else None, _ptr(y) if len(y) else None, len(x), ctypes.byref(out)))
    return out


def kendall_arrays_host(x, y, device=0):
    """st_kendall_arrays_host: the same counts by the GPU path -- both arrays are uploaded to ``device`` and go through the
    sort and count kernels of the compare path."""
    x, y = _float_columns(x, y)
    out = KendallCounts()
    check(load().st_kendall_arrays_host(int(device), _ptr(x) if len(x) else None, _ptr(y) if len(y) else None, len(x), ctypes.byref(out)))
    return out


class TreeInfo(ctypes.Structure):
    _fields_ = [
        ("n_nodes", ctypes.c_int64),
        ("n_leaves", ctypes.c_int64),
        ("root", ctypes.c_int32),
        ("depth", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("strategy", ctypes.c_int32),
        ("canopy_nodes", ctypes.c_int32),
        ("understory_max", ctypes.c_int32),
        ("record_bytes", ctypes.c_int32),
        ("n_devices", ctypes.c_int32),
        ("device_bytes", ctypes.c_int64),
        ("lineage_entries", ctypes.c_int64),
        ("big_batch_kernel", ctypes.c_int32),
        ("tuned", ctypes.c_int32),
        ("host_wire_bytes_in", ctypes.c_int32),
        ("host_wire_bytes_out", ctypes.c_int32),
        ("a_side_bytes", ctypes.c_int32),
        ("dropped_tables", ctypes.c_int32),
        ("table_budget_bytes", ctypes.c_int64),
        ("b_table_bytes_per_leaf", ctypes.c_int32),
        ("ladder_sums", ctypes.c_int32),
        ("ladder_sums_max_pairs", ctypes.c_int64),
        ("heap_lines", ctypes.c_int64),
        ("stream_hint", ctypes.c_int64),
        ("heap_codes", ctypes.c_int64),
    ]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_}
        d["strategy"] = STRATEGY_NAME.get(d["strategy"], str(d["strategy"]))
        d["big_batch_kernel"] = BIG_BATCH_KERNEL.get(d["big_batch_kernel"], str(d["big_batch_kernel"]))
        d["dropped_tables"] = dropped_table_names(d["dropped_tables"])
        return d


_lib = None
_lock = threading.Lock()
_gpu_pid = None     # pid of the process in which this module first put a tree on a GPU


def _check_fork():
    """HIP cannot be used in a child forked after the parent initialised the GPU runtime (its
    worker threads and its device context do not survive fork).  The reference's documented
    recipe -- module-level trees used from multiprocessing.Pool workers
    (docs/examples/SuchTree_examples.md:462-497) -- therefore works when the parent has not
    touched the GPU before the pool forks (uploads are lazy: each worker uploads at its first
    query), or with the 'spawn' start method (trees pickle as their flat arrays)."""
    if _gpu_pid is not None and _gpu_pid != os.getpid():
        raise HipBackendError(
            "this process was forked after its parent (pid %d) had initialised the GPU; HIP cannot be used "
            "in a forked child. Use multiprocessing.get_context('spawn'), or fork the workers before the "
            "first GPU query (a SuchTree uploads lazily, at its first query in each process)." % _gpu_pid)


def _preload_hip_runtime():
    """Make this library and PyTorch agree on ONE HIP runtime, whichever is imported first.

    PyTorch-ROCm wheels bundle their own libamdhip64.so with the same SONAME as the system
    one.  If this library pulled in /opt/rocm's copy first, a later ``import torch`` would
    mix two ROCm stacks in one process and see no device.  So when torch is installed but
    not yet imported, its bundled runtime is loaded first (RTLD_GLOBAL); libsuchtree_hip.so's
    NEEDED libamdhip64.so.7 then resolves to it, exactly as when torch was imported first.
    """
    import sys
    if "torch" in sys.modules or os.environ.get("SUCHTREE_AMD_SYSTEM_HIP", "0") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass   # fall back to the system runtime through the library's RPATH


def load():
    """Load the HIP library once; raise HipBackendError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        autobuild = os.environ.get("SUCHTREE_AMD_AUTOBUILD", "1") != "0"
        try:
            from . import build as _build
            is_stale = os.path.exists(LIB_PATH) and _build.stale()
        except OSError:      # sources not shipped: nothing to compare with
            is_stale = False
        if (not os.path.exists(LIB_PATH) or is_stale) and autobuild:
            # source checkout without the built library, or sources newer than it (the C ABI's
            # struct layout and argtypes are mirrored by hand below): compile (hipcc, gfx950)
            try:
                from . import build as _build
                _build.build()
            except Exception as e:   # no hipcc / compile error: reported below
                build_error = e
            else:
                build_error = None
        else:
            build_error = None
        if os.path.exists(LIB_PATH) and is_stale and build_error is not None:
            import warnings
            warnings.warn("libsuchtree_hip.so is older than its sources and rebuilding failed (%s); "
                          "loading the stale library" % build_error, RuntimeWarning)
        if not os.path.exists(LIB_PATH):
            if build_error is not None:
                raise HipBackendError("libsuchtree_hip.so is not built and building it failed: %s" % build_error)
            raise HipBackendError(
                "libsuchtree_hip.so is not built (%s). Build it with `python -m suchtree_amd.build` "
                "(hipcc, gfx950); this package has no CPU fallback." % LIB_PATH)
        _preload_hip_runtime()
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise HipBackendError("cannot load %s: %s" % (LIB_PATH, e)) from e
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.st_last_error.argtypes = []
        L.st_last_error.restype = ctypes.c_char_p
        L.st_device_count.argtypes = [ctypes.POINTER(i32)]
        L.st_tree_create.argtypes = [vp, vp, i64, i32, i32, ctypes.POINTER(vp)]
        L.st_tree_create_multi.argtypes = [vp, vp, i64, ctypes.POINTER(i32), i32, i32, ctypes.POINTER(vp)]
        L.st_tree_create_ex.argtypes = [vp, vp, i64, ctypes.POINTER(i32), i32, i32, ctypes.POINTER(TreeOptions), ctypes.POINTER(vp)]
        L.st_host_table_plan.argtypes = [vp, vp, i64, i32, i64, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.st_tree_devices.argtypes = [vp, ctypes.POINTER(i32), i32, ctypes.POINTER(i32)]
        L.st_host_chunk_plan.argtypes = [i64, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.st_host_chunk_owner.argtypes = [i64, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.st_tree_destroy.argtypes = [vp]
        L.st_tree_destroy.restype = None
        L.st_tree_info_get.argtypes = [vp, ctypes.POINTER(TreeInfo)]
        L.st_tree_info_get_sized.argtypes = [vp, vp, i64]
        L.st_api_version.argtypes = []
        if L.st_api_version() != API_VERSION:
            raise HipBackendError("libsuchtree_hip.so speaks ABI version %d, this binding %d (include/suchtree_hip.h: ST_API_VERSION); "
                                  "rebuild the library" % (L.st_api_version(), API_VERSION))
        L.st_distances_host.argtypes = [vp, vp, i64, i64, i64, vp, vp, ctypes.POINTER(i64)]
        L.st_distances_host_i32.argtypes = [vp, vp, i64, i64, i64, vp, vp, ctypes.POINTER(i64)]
        L.st_distances_device.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
        L.st_distances_device_f32.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
        L.st_distances_device_wire.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
        L.st_unpack_mrca24_device.argtypes = [i32, vp, i64, vp, vp]
        L.st_fault_check.argtypes = [vp, vp, ctypes.POINTER(i64)]
        L.st_probe_last_choice.argtypes = [vp, vp, ctypes.POINTER(i32)]
        L.st_tree_set_strategy.argtypes = [vp, i32]
        L.st_tree_set_option.argtypes = [vp, ctypes.c_char_p, i64]
        L.st_triangle_device.argtypes = [vp, vp, i64, i64, i64, i64, vp, vp, vp]
        L.st_triangle_host.argtypes = [vp, vp, i64, i64, i64, i64, vp, vp, ctypes.POINTER(i64)]
        L.st_grid_host.argtypes = [vp, vp, i64, vp, i64, i32, i64, i64, vp, vp, ctypes.POINTER(i64)]
        L.st_knn_host.argtypes = [vp, vp, i64, vp, i64, i32, i32, vp, vp, ctypes.POINTER(i64)]
        L.st_quartets_host.argtypes = [vp, vp, i64, i64, i64, vp, ctypes.POINTER(i64)]
        L.st_compare_triangle_host.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, ctypes.c_int32, vp, ctypes.c_int32,
                                               ctypes.POINTER(PairMoments), vp, ctypes.POINTER(i64)]
        L.st_compare_pairs_host.argtypes = [vp, vp, vp, vp, i64, vp, ctypes.c_int32, vp, ctypes.c_int32,
                                            ctypes.POINTER(PairMoments), vp, ctypes.POINTER(i64)]
        L.st_compare_triangle_ranks_host.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, ctypes.POINTER(PairMoments),
                                                     ctypes.POINTER(RankSums), ctypes.POINTER(i64)]
        L.st_compare_pairs_ranks_host.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.POINTER(PairMoments), ctypes.POINTER(RankSums),
                                                  ctypes.POINTER(i64)]
        L.st_spearman_host.argtypes = [vp, vp, i64, ctypes.POINTER(RankSums)]
        L.st_compare_triangle_kendall_host.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, ctypes.POINTER(PairMoments),
                                                       ctypes.POINTER(KendallCounts), ctypes.POINTER(i64)]
        L.st_compare_pairs_kendall_host.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.POINTER(PairMoments), ctypes.POINTER(KendallCounts),
                                                    ctypes.POINTER(i64)]
        L.st_kendall_arrays_host.argtypes = [i32, vp, vp, i64, ctypes.POINTER(KendallCounts)]
        L.st_kendall_host.argtypes = [vp, vp, i64, ctypes.POINTER(KendallCounts)]
        L.st_quartet_positions.argtypes = [i32, i32, ctypes.c_uint64, i64, i64, i64, vp]
        L.st_compare_quartets_leaves_host.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, i64, i64,
                                                      ctypes.POINTER(QuartetTable), ctypes.POINTER(i64)]
        L.st_compare_quartets_host.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.POINTER(QuartetTable), ctypes.POINTER(i64)]
        L.st_hommola_permutation.argtypes = [i32, ctypes.c_uint64, ctypes.c_int32, i64, i32, ctypes.c_int32, vp]
        L.st_hommola_clades_host.argtypes = [vp, vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp, i64, vp, i64, i64, ctypes.c_uint64, i64, vp,
                                             ctypes.POINTER(i64)]
        L.st_partner_dispersion_host.argtypes = [vp, vp, ctypes.c_int32, vp, i64, vp, i64, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp,
                                                 ctypes.POINTER(i64)]
        L.st_dispersion_matrix.argtypes = [i32, vp, ctypes.c_int32, vp, i64, vp, i64, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp]
        L.st_swap_null_tables.argtypes = [i32, ctypes.c_int32, vp, i64, vp, i64, i64, i64, i64, ctypes.c_uint64, ctypes.c_int32, vp, vp]
        L.st_swap_null_schedule.argtypes = [ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_uint64, ctypes.c_int32, vp, ctypes.POINTER(i64),
                                            ctypes.POINTER(i64)]
        L.st_dispersion_matrix_swap.argtypes = [i32, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp, vp]
        L.st_partner_dispersion_swap_host.argtypes = [vp, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp, vp,
                                                      ctypes.POINTER(i64)]
        L.st_beta_dispersion_host.argtypes = [vp, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_int32, i64, ctypes.c_uint64,
                                              ctypes.c_int32, i64, vp, ctypes.POINTER(i64)]
        L.st_beta_dispersion_matrix.argtypes = [i32, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_int32, i64, ctypes.c_uint64,
                                                ctypes.c_int32, i64, vp]
        L.st_unifrac_host.argtypes = [vp, i64, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_int32, i64, vp, vp,
                                      ctypes.POINTER(ctypes.c_int32), vp, vp, ctypes.POINTER(i64)]
        L.st_unifrac_depths.argtypes = [i32, vp, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, i64, vp, vp]
        L.st_unifrac_null_host.argtypes = [vp, i64, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, ctypes.c_int32, i64, ctypes.c_uint64,
                                           ctypes.c_int32, i64, vp, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]
        L.st_unifrac_null_depths.argtypes = [i32, vp, vp, ctypes.c_int32, vp, i64, vp, i64, i64, i64, i64, ctypes.c_uint64, ctypes.c_int32, i64,
                                             vp, vp]
        L.st_unifrac_quantise.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, ctypes.POINTER(ctypes.c_int32)]
        L.st_mantel_codes.argtypes = [i32, vp, vp, vp, ctypes.c_int32, i64, ctypes.c_uint64, ctypes.c_int32, i64, ctypes.POINTER(MantelMoments), vp]
        L.st_mantel_quantise.argtypes = [vp, i64, ctypes.c_int32, vp, ctypes.POINTER(ctypes.c_int32)]
        L.st_group_sums_codes.argtypes = [i32, vp, ctypes.c_int32, vp, ctypes.c_int32, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp]
        L.st_class_sums_codes.argtypes = [i32, vp, vp, ctypes.c_int32, ctypes.c_int32, i64, ctypes.c_uint64, ctypes.c_int32, i64, vp]
        L.st_parafit_codes.argtypes = [i32, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp, ctypes.c_int32, vp, i64, ctypes.c_uint64, i64, vp, vp, vp, vp]
        L.st_clade_ranges.argtypes = [vp, i64, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(i64)]
        L.st_clade_match.argtypes = [i32, ctypes.c_int32, vp, vp, vp, ctypes.c_int32, vp, vp, ctypes.c_int32, ctypes.c_int32, i64, vp, vp, vp]
        L.st_linkage_codes.argtypes = [i32, vp, ctypes.c_int32, vp, ctypes.c_int32, vp]
        L.st_rf_tasks.argtypes = [i32, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp, vp, i64, i64, i64, vp, vp]
        L.st_clade_plan.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i64),
                                    ctypes.POINTER(i64)]
        L.st_compare_clades_host.argtypes = [vp, vp, vp, i64, vp, vp, i64, i64, i64, vp, vp, ctypes.POINTER(i64)]
        L.st_compare_rows_host.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, ctypes.POINTER(i64)]
        L.st_graph_matrices_host.argtypes = [i32, i64, i64, vp, vp, vp, vp, vp]
        L.st_newick_open.argtypes = [ctypes.c_char_p, i64, ctypes.POINTER(vp), ctypes.POINTER(i64),
                                     ctypes.POINTER(i64), ctypes.POINTER(i64),
                                     ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        L.st_newick_fill.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.st_newick_close.argtypes = [vp]
        L.st_newick_close.restype = None
        L.st_host_depths.argtypes = [vp, i64, vp, ctypes.POINTER(ctypes.c_int32)]
        L.st_link_sample_pairs.argtypes = [ctypes.POINTER(ctypes.c_uint64), vp, i64, i64, vp, vp]
        L.st_bucket_moments.argtypes = [vp, i64, i64, vp, vp]
        L.st_device_malloc.argtypes = [i32, i64, ctypes.POINTER(vp)]
        L.st_device_free.argtypes = [i32, vp]
        L.st_memcpy_h2d.argtypes = [i32, vp, vp, i64]
        L.st_memcpy_d2h.argtypes = [i32, vp, vp, i64]
        L.st_device_synchronize.argtypes = [i32]
        for name in SYMBOLS:
            if name not in ("st_last_error", "st_tree_destroy", "st_newick_close"):
                getattr(L, name).restype = i32
        _lib = L
    return _lib


class MeasureOnly(HipBackendError):
    """A host-path call made under the handle option ``measure`` (2 / 4) skipped part of the pipeline: its time counts,
    its results do not (bench_legs.host_path_leg)."""


def last_error():
    return load().st_last_error().decode("utf-8", "replace")


def check(rc, tree_size=None, bad_id=None):
    """Map a C return code onto the package's exceptions."""
    if rc == ST_OK:
        return
    msg = last_error()
    if rc == ST_ERR_BOUNDS:
        raise InvalidNodeError(bad_id, tree_size)
    if rc == ST_ERR_TREE:
        raise TreeStructureError(msg)
    if rc == ST_ERR_ARG:
        raise ValueError(msg)
    if rc == ST_ERR_NOMEM:
        raise MemoryError(msg)
    if rc == ST_ERR_MEASURE_ONLY:
        raise MeasureOnly(msg)
    raise HipBackendError(msg)


def graph_matrices(n, u, v, w, device=0, want_adjacency=True, want_laplacian=True):
    """Dense adjacency / Laplacian (n x n float64) of an undirected weighted edge list, on the GPU."""
    L = load()
    u = np.ascontiguousarray(u, dtype=np.int32)
    v = np.ascontiguousarray(v, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    adj = np.empty((n, n), dtype=np.float64) if want_adjacency else None
    lap = np.empty((n, n), dtype=np.float64) if want_laplacian else None
    check(L.st_graph_matrices_host(int(device), int(n), int(len(u)), _ptr(u), _ptr(v), _ptr(w), _ptr(adj), _ptr(lap)))
    return adj, lap


def newick_native(text):
    """Parse with the native ingest; returns a dict of arrays or None when the native
    parser declines (the pure-Python parser then handles -- and diagnoses -- the input)."""
    try:
        L = load()
    except HipBackendError:
        return None
    try:
        raw = text.encode("ascii")
    except UnicodeEncodeError:
        return None
    h = ctypes.c_void_p()
    n, nl, nb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    root, depth = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = L.st_newick_open(raw, len(raw), ctypes.byref(h), ctypes.byref(n), ctypes.byref(nl), ctypes.byref(nb),
                          ctypes.byref(root), ctypes.byref(depth))
    if rc != ST_OK:
        return None
    try:
        n, nl, nb = n.value, nl.value, nb.value
        out = {k: np.empty(n, dtype=np.int32) for k in ("parent", "left", "right")}
        out["support"] = np.empty(n, dtype=np.float32)
        out["distance"] = np.empty(n, dtype=np.float32)
        out["leaf_ids"] = np.empty(nl, dtype=np.int32)
        names = ctypes.create_string_buffer(max(nb, 1))
        offs = np.empty(nl + 1, dtype=np.int64)
        check(L.st_newick_fill(h, _ptr(out["parent"]), _ptr(out["left"]), _ptr(out["right"]),
                               _ptr(out["support"]), _ptr(out["distance"]), _ptr(out["leaf_ids"]),
                               ctypes.cast(names, ctypes.c_void_p), _ptr(offs)))
        blob = names.raw[:nb].decode("ascii")
        o = offs.tolist()
        out["names"] = [blob[o[i]:o[i + 1]] for i in range(nl)]
        out["root"], out["depth"] = int(root.value), int(depth.value)
        return out
    finally:
        L.st_newick_close(h)


def link_sample_pairs(state, linklist, count):
    """(query_a, query_b, new_state): `count` link-pair draws of the reference's xorshift64* generator
    (st_link_sample_pairs; MuchTree.pyx:2937-2949, 3025-3038).  Host only."""
    ll = np.ascontiguousarray(linklist, dtype=np.int64)
    qa = np.empty((int(count), 2), dtype=np.int64)
    qb = np.empty((int(count), 2), dtype=np.int64)
    st = ctypes.c_uint64(int(state) & 0xFFFFFFFFFFFFFFFF)
    check(load().st_link_sample_pairs(ctypes.byref(st), ll.ctypes.data, int(ll.shape[0]), int(count), qa.ctypes.data, qb.ctypes.data))
    return qa, qb, int(st.value)


def bucket_moments(dist, sums, sumsq):
    """sums[i] += d, sumsq[i] += pow(d, 2.0) over the rows of `dist` (buckets, n), in place (st_bucket_moments)."""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    assert sums.dtype == np.float64 and sumsq.dtype == np.float64 and sums.flags.c_contiguous and sumsq.flags.c_contiguous
    check(load().st_bucket_moments(d.ctypes.data, int(d.shape[0]), int(d.shape[1]), sums.ctypes.data, sumsq.ctypes.data))


def host_chunk_map(n, n_devices):
    """[(device_index, first_pair, n_pairs)] for every pipeline chunk of an n-pair host batch
    dealt over n_devices GPUs (st_host_chunk_plan / st_host_chunk_owner; no GPU needed)."""
    L = load()
    chunk, count = ctypes.c_int64(0), ctypes.c_int64(0)
    check(L.st_host_chunk_plan(int(n), int(n_devices), ctypes.byref(chunk), ctypes.byref(count)))
    out = []
    for c in range(count.value):
        d, first, m = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(L.st_host_chunk_owner(int(n), int(n_devices), c, ctypes.byref(d), ctypes.byref(first), ctypes.byref(m)))
        out.append((int(d.value), int(first.value), int(m.value)))
    return out


class _LentBlock:
    """An ordinary (pageable) block on loan to one numpy array; see RecyclePool."""

    def __init__(self, pool, block, n, dtype):
        self._pool, self._block = pool, block
        self.__array_interface__ = {"data": (block.ctypes.data, False), "shape": (n,), "typestr": np.dtype(dtype).str, "version": 3}

    def __del__(self):
        try:
            self._pool._give_back(self._block)
        except Exception:     # interpreter shutdown
            pass


class RecyclePool:
    """Recycled ordinary memory for LARGE result arrays.

    What a fresh numpy array costs beyond 32 MiB -- where glibc stops recycling freed blocks and
    maps / unmaps every one -- is the kernel zeroing its pages on first touch and tearing them
    down on release: for 5e7 pairs (600 MB of float64 + int32) three times as long as the
    computation (``profiles/host_path_r02.jsonl``: 1.2e9 pairs/s for
    "call, drop the result" against 4.8e9 into arrays that are reused).  Result arrays of that
    size are therefore handed out as views of blocks that come back here when the array and all
    its views are gone, and go out again, resident, with the next call.  The memory is ordinary:
    readable in ``fork()`` children, swappable, and returned to the system by ``trim()``.
    ``SUCHTREE_AMD_RECYCLE_MB`` caps what the pool may hold (default 2048; 0 switches it off);
    beyond the cap callers get plain ``np.empty`` arrays.
    """

    MIN_BYTES = 32 << 20

    def __init__(self, budget_bytes=None):
        if budget_bytes is None:
            budget_bytes = int(os.environ.get("SUCHTREE_AMD_RECYCLE_MB", "2048")) << 20
        self.budget = int(budget_bytes)
        self.total = 0
        self._free = {}
        # re-entrant: the garbage collector may run a lent block's __del__ (-> _give_back) on this
        # very thread while it is inside array() / _give_back()
        self._lock = threading.RLock()

    @staticmethod
    def _size_class(nbytes):
        cap = 1 << 21
        while cap < nbytes and cap < (1 << 26):
            cap <<= 1
        if cap < nbytes:                                   # beyond 64 MiB: multiples of 64 MiB
            cap = (nbytes + (1 << 26) - 1) >> 26 << 26
        return cap

    def array(self, n, dtype):
        """A 1-D array of ``n`` items in a recycled block, or None (too small, over budget)."""
        nbytes = int(n) * np.dtype(dtype).itemsize
        if nbytes < self.MIN_BYTES or self.budget <= 0:
            return None
        cap = self._size_class(nbytes)
        with self._lock:
            stack = self._free.get(cap)
            block = stack.pop() if stack else None
            if block is None:
                if self.total + cap > self.budget:
                    return None
                self.total += cap
        if block is None:
            block = np.empty(cap, dtype=np.uint8)
        return np.asarray(_LentBlock(self, block, int(n), dtype))

    def _give_back(self, block):
        with self._lock:
            self._free.setdefault(block.nbytes, []).append(block)

    def trim(self):
        """Release every block that is not on loan."""
        with self._lock:
            free, self._free = self._free, {}
            for cap, blocks in free.items():
                self.total -= cap * len(blocks)


_recycle_pool = None


def recycle_pool():
    global _recycle_pool
    if _recycle_pool is None:
        _recycle_pool = RecyclePool()
    return _recycle_pool


def device_count():
    c = ctypes.c_int(0)
    rc = load().st_device_count(ctypes.byref(c))
    if rc != ST_OK:
        return 0
    return int(c.value)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _arg(a):
    """A call's argument: an array goes as its pointer (NULL when it is empty or None), a result structure by reference,
    anything else as it is."""
    if isinstance(a, np.ndarray):
        return _ptr(a) if a.size else None
    return ctypes.byref(a) if isinstance(a, ctypes.Structure) else a


def clade_plan(parent, link_leaf, max_links=None):
    """st_clade_plan (host only): the clade-contiguous permutation of the links (given in rank order by their clade-tree
    leaf id), each node's link range / count / leaf count, the segments (a CLADE_SEGMENT array in pair order) and the
    pair count.  Returns a dict of numpy arrays and ints."""
    L = load()
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    link_leaf = np.ascontiguousarray(link_leaf, dtype=np.int64)
    n, m = int(parent.shape[0]), int(link_leaf.shape[0])
    perm = np.empty(m, dtype=np.int64)
    begin, count, leaves = (np.empty(n, dtype=np.int64) for _ in range(3))
    segs = np.empty(2 * max(n, 1), dtype=CLADE_SEGMENT)
    n_segs, total, bad = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = L.st_clade_plan(_ptr(parent), n, _ptr(link_leaf) if m else None, m, -1 if max_links is None else int(max_links),
                         _ptr(perm) if m else None, _ptr(begin), _ptr(count), _ptr(leaves), _ptr(segs), len(segs),
                         ctypes.byref(n_segs), ctypes.byref(total), ctypes.byref(bad))
    check(rc, tree_size=n, bad_id=int(bad.value))
    return {"perm": perm, "begin": begin, "count": count, "leaves": leaves, "segments": segs[: n_segs.value].copy(),
            "total_pairs": int(total.value)}


def host_table_plan(parent, distance, strategy="auto", table_mb=0):
    """What a tree would get on the device under a table budget (MiB; 0 = SUCHTREE_AMD_TABLE_MB if set, else none),
    computed on the host (no GPU): ``{"device_bytes", "dropped_tables", "family"}`` (st_host_table_plan)."""
    L = load()
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    distance = np.ascontiguousarray(distance, dtype=np.float32)
    b, d, f = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
    check(L.st_host_table_plan(_ptr(parent), _ptr(distance), int(parent.shape[0]), STRATEGY[strategy], int(float(table_mb) * (1 << 20)),
                               ctypes.byref(b), ctypes.byref(d), ctypes.byref(f)))
    return {"device_bytes": int(b.value), "dropped_tables": dropped_table_names(int(d.value)), "family": STRATEGY_NAME.get(int(f.value))}


class DeviceTree:
    """Owner of one ``st_tree`` handle: the tree resident in one GPU's HBM, or -- with
    ``devices=[...]`` -- replicated on several GPUs of the node (``st_tree_create_multi``),
    the host-buffer entry points then dealing their chunks over all of them."""

    def __init__(self, parent, distance, device=0, strategy="auto", devices=None, table_mb=None):
        """``table_mb``: budget (MiB) for the tree's device tables (st_tree_options.table_budget_bytes; default: the
        environment's SUCHTREE_AMD_TABLE_MB, else none): accelerator tables are left out, in a stated order, until the
        rest fits -- ``info()["dropped_tables"]`` names them; results are the same bits."""
        global _gpu_pid
        _check_fork()
        L = load()
        self._lib = L
        self._h = ctypes.c_void_p()
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        distance = np.ascontiguousarray(distance, dtype=np.float32)
        if parent.ndim != 1 or parent.shape != distance.shape:
            raise ValueError("parent and distance must be 1-D arrays of equal length")
        if strategy not in STRATEGY:
            raise ValueError("strategy must be one of %s" % sorted(STRATEGY))
        self.size = int(parent.shape[0])
        self._pid = os.getpid()
        if devices is not None or table_mb is not None:
            devices = [int(d) for d in (devices if devices is not None else [device])]
            if not devices:
                raise ValueError("devices must not be empty")
            arr = (ctypes.c_int * len(devices))(*devices)
            opts = TreeOptions()
            if table_mb is not None:
                if table_mb < 0:
                    raise ValueError("table_mb must be >= 0")
                opts.table_budget_bytes = int(float(table_mb) * (1 << 20))
            rc = L.st_tree_create_ex(_ptr(parent), _ptr(distance), self.size, arr, len(devices),
                                     STRATEGY[strategy], ctypes.byref(opts), ctypes.byref(self._h))
            device = devices[0]
        else:
            rc = L.st_tree_create(_ptr(parent), _ptr(distance), self.size, int(device),
                                  STRATEGY[strategy], ctypes.byref(self._h))
            devices = [int(device)]
        check(rc)
        self.device = int(device)
        self.devices = list(devices)
        if _gpu_pid is None:
            _gpu_pid = self._pid

    def close(self):
        h, self._h = self._h, ctypes.c_void_p()
        if h and self._pid == os.getpid():     # a handle inherited through fork is not ours to destroy
            self._lib.st_tree_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise HipBackendError("tree handle is closed")
        if self._pid != os.getpid():
            _check_fork()
            raise HipBackendError("tree handle belongs to another process (pid %d)" % self._pid)
        return self._h

    def info(self):
        ti = TreeInfo()
        check(self._lib.st_tree_info_get_sized(self.handle, ctypes.byref(ti), ctypes.sizeof(ti)))
        return ti.as_dict()

    def set_strategy(self, strategy):
        check(self._lib.st_tree_set_strategy(self.handle, STRATEGY[strategy]))

    def set_option(self, name, value):
        check(self._lib.st_tree_set_option(self.handle, name.encode(), int(value)))

    def _out(self, buf, n, dtype, want):
        if not want:
            return None
        if buf is None:
            arr = recycle_pool().array(n, dtype)
            if arr is not None:
                return arr
            return np.empty(n, dtype=dtype)
        if buf.dtype != dtype or buf.shape != (n,) or not buf.flags.c_contiguous:
            raise ValueError("output buffer must be a contiguous %s array of shape (%d,)" % (np.dtype(dtype).name, n))
        return buf

    def distances_host(self, pairs, want_dist=True, want_mrca=False, out_dist=None, out_mrca=None):
        """pairs: int64 (n,2) ndarray with any strides (multiples of 8 bytes).
        ``out_dist`` / ``out_mrca``: optional preallocated result arrays (reused buffers
        avoid the page-fault cost of fresh memory on every call)."""
        n = int(pairs.shape[0])
        out_d = self._out(out_dist, n, np.float64, want_dist)
        out_m = self._out(out_mrca, n, np.int32, want_mrca)
        if n == 0:
            return out_d, out_m
        item = pairs.dtype.itemsize
        if pairs.dtype not in (np.int64, np.int32):
            raise ValueError("pairs must be int64 or int32")
        if pairs.strides[0] % item or pairs.strides[1] % item:
            pairs = np.ascontiguousarray(pairs)
        s0, s1 = pairs.strides[0] // item, pairs.strides[1] // item
        if s0 < 0 or s1 < 0:   # negative strides: the base pointer is not the lowest address
            pairs = np.ascontiguousarray(pairs)
            s0, s1 = 2, 1
        bad = ctypes.c_int64(0)
        fn = self._lib.st_distances_host if item == 8 else self._lib.st_distances_host_i32
        rc = fn(self.handle, _ptr(pairs), n, s0, s1, _ptr(out_d), _ptr(out_m),
                                         ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out_d, out_m

    def triangle_host(self, ids, k_begin=0, k_count=None, want_dist=True, want_mrca=False,
                      out_dist=None, out_mrca=None):
        """Lower-triangle all-pairs over ``ids`` (1-D int64): pair k = (ids[j], ids[i]),
        k = i(i-1)/2 + j; returns the slice [k_begin, k_begin + k_count)."""
        ids = np.asarray(ids)
        if ids.ndim != 1:
            raise ValueError("ids must be 1-D")
        if ids.dtype != np.int64 or ids.strides[0] % 8 or ids.strides[0] < 0:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
        m = int(ids.shape[0])
        total = m * (m - 1) // 2
        if k_count is None:
            k_count = total - k_begin
        out_d = self._out(out_dist, k_count, np.float64, want_dist)
        out_m = self._out(out_mrca, k_count, np.int32, want_mrca)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_triangle_host(self.handle, _ptr(ids) if m else None, m,
                                        ids.strides[0] // 8 if m else 1, int(k_begin), int(k_count),
                                        _ptr(out_d), _ptr(out_m), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out_d, out_m

    def grid_host(self, row_ids, col_ids, symmetric=False, e_begin=0, e_count=None, want_dist=True,
                  want_mrca=False, out_dist=None, out_mrca=None):
        """Element e = r * len(col_ids) + c of the grid is the pair (row_ids[r], col_ids[c]);
        ``symmetric`` (same list twice): below the diagonal the mirror image's argument order,
        i.e. the full range is the symmetric matrix of pairwise_distances, flattened."""
        row_ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        col_ids = np.ascontiguousarray(col_ids, dtype=np.int64)
        if row_ids.ndim != 1 or col_ids.ndim != 1:
            raise ValueError("id lists must be 1-D")
        total = int(row_ids.shape[0]) * int(col_ids.shape[0])
        if e_count is None:
            e_count = total - e_begin
        out_d = self._out(out_dist, e_count, np.float64, want_dist)
        out_m = self._out(out_mrca, e_count, np.int32, want_mrca)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_grid_host(self.handle, _ptr(row_ids) if len(row_ids) else None, len(row_ids),
                                    _ptr(col_ids) if len(col_ids) else None, len(col_ids), int(bool(symmetric)),
                                    int(e_begin), int(e_count), _ptr(out_d), _ptr(out_m), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out_d, out_m

    KNN_MAX_K = 256

    def knn_host(self, queries, cands, k, skip_self=False):
        """(index int64 (q,k) into cands, dist float64 (q,k)): the k nearest candidates of every
        query, selected on the GPU; -1 / NaN where fewer than k candidates exist."""
        queries = np.ascontiguousarray(queries, dtype=np.int64)
        cands = np.ascontiguousarray(cands, dtype=np.int64)
        if queries.ndim != 1 or cands.ndim != 1:
            raise ValueError("queries and cands must be 1-D")
        q = int(queries.shape[0])
        idx = np.empty((q, int(k)), dtype=np.int64)
        dist = np.empty((q, int(k)), dtype=np.float64)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_knn_host(self.handle, _ptr(queries) if q else None, q, _ptr(cands) if len(cands) else None,
                                   len(cands), int(k), int(bool(skip_self)), _ptr(idx), _ptr(dist), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return idx, dist

    def quartets_host(self, quartets):
        """quartets: int64 (n,4) ndarray (any non-negative strides); returns int64 (n,4)."""
        n = int(quartets.shape[0])
        flat = recycle_pool().array(4 * n, np.int64)      # (large results: recycled blocks)
        out = flat.reshape(n, 4) if flat is not None else np.empty((n, 4), dtype=np.int64)
        if n == 0:
            return out
        if quartets.strides[0] % 8 or quartets.strides[1] % 8 or quartets.strides[0] < 0 or quartets.strides[1] < 0:
            quartets = np.ascontiguousarray(quartets)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_quartets_host(self.handle, _ptr(quartets), n, quartets.strides[0] // 8,
                                        quartets.strides[1] // 8, _ptr(out), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out

    def _compare_check(self, other, rc, bad):
        bad = int(bad.value)
        if rc == ST_ERR_BOUNDS and 0 <= bad < self.size:      # (tree_x's ids are checked first: an id valid there is tree_y's)
            check(rc, tree_size=other.size, bad_id=bad)
        check(rc, tree_size=self.size, bad_id=bad)

    @staticmethod
    def _compare_hist(edges):
        """(edges_x, bins_x, edges_y, bins_y, hist) ctypes arguments; edges = None or (xedges, yedges) float64."""
        if edges is None:
            return None, 0, None, 0, None
        ex = np.ascontiguousarray(edges[0], dtype=np.float64)
        ey = np.ascontiguousarray(edges[1], dtype=np.float64)
        if ex.ndim != 1 or ey.ndim != 1 or len(ex) < 2 or len(ey) < 2:
            raise ValueError("histogram edges must be 1-D arrays of at least two values")
        bx, by = len(ex) - 1, len(ey) - 1
        if bx * by > 16384:      # (checked again by the library, before anything is allocated here)
            raise ValueError("histogram of %d cells: at most 16384" % (bx * by))
        return ex, bx, ey, by, np.zeros((bx, by), dtype=np.int64)

    @staticmethod
    def _id_lists(ids_x, ids_y):
        """(ids_x, ids_y, m): two aligned id lists as contiguous 1-D int64 arrays, and their length."""
        ids_x = np.ascontiguousarray(ids_x, dtype=np.int64)
        ids_y = np.ascontiguousarray(ids_y, dtype=np.int64)
        if ids_x.ndim != 1 or ids_x.shape != ids_y.shape:
            raise ValueError("ids_x and ids_y must be 1-D arrays of equal length")
        return ids_x, ids_y, int(ids_x.shape[0])

    @staticmethod
    def _id_rows(rows_x, rows_y, k, what):
        """(rows_x, rows_y, n): two aligned (n, k) id arrays -- ``what`` "pairs" (k = 2) or "quartets" (k = 4) -- as
        contiguous int64 arrays, and their row count."""
        rows_x = np.ascontiguousarray(rows_x, dtype=np.int64)
        rows_y = np.ascontiguousarray(rows_y, dtype=np.int64)
        if rows_x.ndim != 2 or rows_x.shape[1:] != (k,) or rows_x.shape != rows_y.shape:
            raise ValueError("%s_x and %s_y must be (n, %d) arrays of equal shape" % (what, what, k))
        return rows_x, rows_y, int(rows_x.shape[0])

    @staticmethod
    def _triangle_count(m, k_begin, k_count):
        """k_count, by default up to the last pair of the triangle over m ids."""
        return int(m * (m - 1) // 2 - int(k_begin) if k_count is None else k_count)

    def _compare_call(self, fn, other, args, *outs):
        """fn(self, other, *args, *outs, &bad_id) of a two-tree entry point, every argument as _arg passes it.  Raises as
        _compare_check does."""
        bad = ctypes.c_int64(0)
        self._compare_check(other, fn(self.handle, other.handle, *(_arg(a) for a in args + outs), ctypes.byref(bad)), bad)

    def compare_triangle_host(self, other, ids_x, ids_y, k_begin=0, k_count=None, edges=None):
        """Moments (``PairMoments``) and, with ``edges = (xedges, yedges)``, the int64 2-D histogram of the distances of
        pairs k in [k_begin, k_begin + k_count) of the triangle over ``ids_x`` in this tree and ``ids_y`` in ``other``
        (st_compare_triangle_host; the pair enumeration of triangle_host).  Returns (moments, hist or None)."""
        ids_x, ids_y, m = self._id_lists(ids_x, ids_y)
        k_count = self._triangle_count(m, k_begin, k_count)
        ex, bx, ey, by, hist = self._compare_hist(edges)
        out = PairMoments()
        self._compare_call(self._lib.st_compare_triangle_host, other, (ids_x, ids_y, m, int(k_begin), k_count, ex, bx, ey, by), out, hist)
        return out, hist

    def compare_pairs_host(self, other, pairs_x, pairs_y, edges=None):
        """The same over explicit pairs: row i of ``pairs_x`` (int64 (n,2)) in this tree, row i of ``pairs_y`` in ``other``
        (st_compare_pairs_host).  Returns (moments, hist or None)."""
        pairs_x, pairs_y, n = self._id_rows(pairs_x, pairs_y, 2, "pairs")
        ex, bx, ey, by, hist = self._compare_hist(edges)
        out = PairMoments()
        self._compare_call(self._lib.st_compare_pairs_host, other, (pairs_x, pairs_y, n, ex, bx, ey, by), out, hist)
        return out, hist

    def compare_triangle_ranks_host(self, other, ids_x, ids_y, k_begin=0, k_count=None, chunk_pairs=0):
        """compare_triangle_host without a histogram plus the exact rank sums of the same pairs
        (st_compare_triangle_ranks_host).  Returns (moments, ``RankSums``)."""
        ids_x, ids_y, m = self._id_lists(ids_x, ids_y)
        out, ranks = PairMoments(), RankSums()
        self._compare_call(self._lib.st_compare_triangle_ranks_host, other,
                           (ids_x, ids_y, m, int(k_begin), self._triangle_count(m, k_begin, k_count), int(chunk_pairs)), out, ranks)
        return out, ranks

    def compare_pairs_ranks_host(self, other, pairs_x, pairs_y, chunk_pairs=0):
        """The same over explicit pairs (st_compare_pairs_ranks_host).  Returns (moments, ``RankSums``)."""
        pairs_x, pairs_y, n = self._id_rows(pairs_x, pairs_y, 2, "pairs")
        out, ranks = PairMoments(), RankSums()
        self._compare_call(self._lib.st_compare_pairs_ranks_host, other, (pairs_x, pairs_y, n, int(chunk_pairs)), out, ranks)
        return out, ranks

    def compare_triangle_kendall_host(self, other, ids_x, ids_y, k_begin=0, k_count=None, chunk_pairs=0):
        """compare_triangle_host without a histogram plus the exact Kendall counts of the same pairs
        (st_compare_triangle_kendall_host).  Returns (moments, ``KendallCounts``)."""
        ids_x, ids_y, m = self._id_lists(ids_x, ids_y)
        out, counts = PairMoments(), KendallCounts()
        self._compare_call(self._lib.st_compare_triangle_kendall_host, other,
                           (ids_x, ids_y, m, int(k_begin), self._triangle_count(m, k_begin, k_count), int(chunk_pairs)), out, counts)
        return out, counts

    def compare_pairs_kendall_host(self, other, pairs_x, pairs_y, chunk_pairs=0):
        """The same over explicit pairs (st_compare_pairs_kendall_host).  Returns (moments, ``KendallCounts``)."""
        pairs_x, pairs_y, n = self._id_rows(pairs_x, pairs_y, 2, "pairs")
        out, counts = PairMoments(), KendallCounts()
        self._compare_call(self._lib.st_compare_pairs_kendall_host, other, (pairs_x, pairs_y, n, int(chunk_pairs)), out, counts)
        return out, counts

    def compare_quartets_leaves_host(self, other, ids_x, ids_y, mode="all", seed=0, k_begin=0, k_count=None, chunk_quartets=0):
        """The int64 (4, 4) table of quartet classes -- [class here][class in ``other``] -- of quartets
        [k_begin, k_begin + k_count) generated on the GPU over the aligned id lists ``ids_x`` (this tree) and ``ids_y``
        (``other``): ``mode`` "all" = the C(m,4) subsets in colexicographic order (k_count None: up to the last),
        "sample" = quartet k drawn from (seed, k, m) (st_compare_quartets_leaves_host)."""
        ids_x, ids_y, m = self._id_lists(ids_x, ids_y)
        if mode not in QUARTET_MODE:
            raise ValueError("mode must be 'all' or 'sample'")
        if k_count is None:
            if mode != "all":
                raise ValueError("a sample needs k_count")
            if m > QUARTET_MAX_LEAVES_ALL:
                raise ValueError("all quartets of %d leaves: at most %d leaves" % (m, QUARTET_MAX_LEAVES_ALL))
            k_count = (m * (m - 1) * (m - 2) * (m - 3) // 24 if m >= 4 else 0) - int(k_begin)
        out = QuartetTable()
        self._compare_call(self._lib.st_compare_quartets_leaves_host, other,
                           (ids_x, ids_y, m, QUARTET_MODE[mode], int(seed) & 0xFFFFFFFFFFFFFFFF, int(k_begin), int(k_count), int(chunk_quartets)),
                           out)
        return out.as_array()

    def compare_quartets_host(self, other, quartets_x, quartets_y, chunk_quartets=0):
        """The same table over explicit quartets: row i of ``quartets_x`` (int64 (n,4)) in this tree against row i of
        ``quartets_y`` in ``other`` (st_compare_quartets_host)."""
        quartets_x, quartets_y, n = self._id_rows(quartets_x, quartets_y, 4, "quartets")
        out = QuartetTable()
        self._compare_call(self._lib.st_compare_quartets_host, other, (quartets_x, quartets_y, n, int(chunk_quartets)), out)
        return out.as_array()

    def compare_clades_host(self, other, parent, ids_x, ids_y, max_links=None, chunk_pairs=0):
        """st_compare_clades_host: one PairMoments-shaped record per node of ``other`` (the clade tree, whose int32
        ``parent`` array is given), x = this tree, y = ``other``, over the links ``ids_x`` / ``ids_y`` (rank order).
        Returns (structured array of st_pair_moments fields, per-node link counts); n = -1 marks a node over
        ``max_links``."""
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        ids_x, ids_y, m = self._id_lists(ids_x, ids_y)
        n = int(parent.shape[0])
        out = np.zeros(n, dtype=PAIR_MOMENTS)
        count = np.zeros(n, dtype=np.int64)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_compare_clades_host(self.handle, other.handle, _ptr(parent), n, _ptr(ids_x) if m else None,
                                              _ptr(ids_y) if m else None, m, -1 if max_links is None else int(max_links),
                                              int(chunk_pairs), _ptr(out), _ptr(count), ctypes.byref(bad))
        bad = int(bad.value)
        if rc == ST_ERR_BOUNDS and not (0 <= bad < self.size):
            check(rc, tree_size=self.size, bad_id=bad)
        check(rc, tree_size=other.size, bad_id=bad)
        return out, count

    def compare_rows_host(self, other, ids_x, ids_y, chunk_pairs=0):
        """st_compare_rows_host: one PairMoments-shaped record per row of the int64 (n_rows, m) ``ids_x`` (this tree) /
        ``ids_y`` (``other``): the moments of the triangle over that row's ids (the enumeration of triangle_host).  A row's
        record depends on its ids alone -- not on its index, the other rows or ``chunk_pairs`` (0 or a multiple of
        CLADE_TILE)."""
        ids_x = np.ascontiguousarray(ids_x, dtype=np.int64)
        ids_y = np.ascontiguousarray(ids_y, dtype=np.int64)
        if ids_x.ndim != 2 or ids_x.shape != ids_y.shape:
            raise ValueError("ids_x and ids_y must be 2-D arrays of equal shape")
        n_rows, m = (int(v) for v in ids_x.shape)
        out = np.zeros(n_rows, dtype=PAIR_MOMENTS)
        self._compare_call(self._lib.st_compare_rows_host, other, (ids_x, ids_y, n_rows, m, int(chunk_pairs)), out)
        return out

    def hommola_clades_host(self, clade_tree, univ_o, univ_c, pos_o, pos_c, clades, permutations, seed, chunk_blocks=0):
        """st_hommola_clades_host: x = this tree (the other tree of the test), y = ``clade_tree``.  ``clades`` is a
        HOMMOLA_CLADE array; returns the (len(clades), permutations + 1) array of st_pair_moments records, row p of every
        clade (p = 0: the links as they are)."""
        univ_o = np.ascontiguousarray(univ_o, dtype=np.int64)
        univ_c = np.ascontiguousarray(univ_c, dtype=np.int64)
        pos_o = np.ascontiguousarray(pos_o, dtype=np.int32)
        pos_c = np.ascontiguousarray(pos_c, dtype=np.int32)
        clades = np.ascontiguousarray(clades, dtype=HOMMOLA_CLADE)
        if univ_o.ndim != 1 or univ_c.ndim != 1 or pos_o.ndim != 1 or pos_o.shape != pos_c.shape or clades.ndim != 1:
            raise ValueError("universes, positions and clades must be 1-D, pos_o and pos_c of equal length")
        out = np.zeros((len(clades), int(permutations) + 1 if int(permutations) >= 0 else 0), dtype=PAIR_MOMENTS)
        self._compare_call(self._lib.st_hommola_clades_host, clade_tree,
                           (univ_o, len(univ_o), univ_c, len(univ_c), pos_o, pos_c, len(pos_o), clades, len(clades), int(permutations),
                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(chunk_blocks)), out)
        return out

    def partner_dispersion_host(self, univ, sets, permutations, seed, stream=0, chunk_tasks=0):
        """st_partner_dispersion_host: the (n_sets, permutations + 1) array of DISPERSION_RECORD of the position sets
        ``sets`` (as in ``dispersion_matrix``) over the universe ``univ`` (node ids of this tree, depth-first)."""
        univ = np.ascontiguousarray(univ, dtype=np.int64)
        if univ.ndim != 1:
            raise ValueError("the universe must be 1-D")
        _dispersion_args(permutations, stream, chunk_tasks)
        pos, off, n_sets = _dispersion_sets(sets, len(univ))
        out = np.zeros((n_sets, int(permutations) + 1), dtype=DISPERSION_RECORD)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_partner_dispersion_host(self.handle, _arg(univ), len(univ), _arg(pos), len(pos), _ptr(off), n_sets, int(permutations),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(chunk_tasks), _arg(out), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out

    def partner_dispersion_swap_host(self, univ, sets, permutations, seed, iterations=None, stream=0, chunk_tasks=0):
        """st_partner_dispersion_swap_host: (records, accepted) of ``partner_dispersion_host`` under the swap null (as
        ``dispersion_matrix_swap``, the matrix written by this tree's distance kernels)."""
        univ = np.ascontiguousarray(univ, dtype=np.int64)
        if univ.ndim != 1:
            raise ValueError("the universe must be 1-D")
        _dispersion_args(permutations, stream, chunk_tasks)
        pos, off, n_sets = _dispersion_sets(sets, len(univ))
        out = np.zeros((n_sets, int(permutations) + 1), dtype=DISPERSION_RECORD)
        accepted = np.zeros(int(permutations) + 1, dtype=np.int64)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_partner_dispersion_swap_host(self.handle, _arg(univ), len(univ), _arg(pos), len(pos), _ptr(off), n_sets, int(permutations),
                                                       swap_iterations(iterations, _swap_links(off)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream),
                                                       int(chunk_tasks), _arg(out), _arg(accepted), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out, accepted

    def beta_dispersion_host(self, univ, sets, begin=0, count=None, exclude_shared=False, permutations=0, seed=0, stream=0, chunk_tasks=0):
        """st_beta_dispersion_host: the (count, 2, permutations + 1) array of DISPERSION_RECORD of pairs [begin, begin + count)
        of the triangle over the position sets ``sets`` (as in ``beta_dispersion_matrix``) over the universe ``univ`` (node
        ids of this tree, depth-first)."""
        univ = np.ascontiguousarray(univ, dtype=np.int64)
        if univ.ndim != 1:
            raise ValueError("the universe must be 1-D")
        _dispersion_args(permutations, stream, chunk_tasks)
        pos, off, n_sets = _dispersion_sets(sets, len(univ))
        begin, count = _unifrac_range(n_sets, begin, count, 0)
        out = np.zeros((count, 2, int(permutations) + 1), dtype=DISPERSION_RECORD)
        bad = ctypes.c_int64(0)
        rc = self._lib.st_beta_dispersion_host(self.handle, _arg(univ), len(univ), _arg(pos), len(pos), _ptr(off), n_sets, begin, count,
                                               int(bool(exclude_shared)), int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream),
                                               int(chunk_tasks), _arg(out), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return out

    def unifrac_host(self, root, univ, sets, begin=0, count=None, shift=None, chunk_pairs=0):
        """st_unifrac_host: (pd_q, union_q, shift, d, h) of the position sets ``sets`` (as in ``dispersion_matrix``) over the
        universe ``univ`` (leaf ids of this tree under ``root``, depth-first): the int64 PD of every set, the union sums of
        pairs [begin, begin + count) of the triangle, the shift used and the float32 depths."""
        univ = np.ascontiguousarray(univ, dtype=np.int64)
        if univ.ndim != 1:
            raise ValueError("the universe must be 1-D")
        n = len(univ)
        pos, off, n_sets = _dispersion_sets(sets, n)
        begin, count = _unifrac_range(n_sets, begin, count, chunk_pairs)
        pd_q, union_q = np.zeros(n_sets, dtype=np.int64), np.zeros(count, dtype=np.int64)
        d, h = np.zeros(n, dtype=np.float32), np.zeros(max(n - 1, 0), dtype=np.float32)
        used, bad = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self._lib.st_unifrac_host(self.handle, int(root), _arg(univ), n, _arg(pos), len(pos), _ptr(off), n_sets, begin, count,
                                       -1 if shift is None else int(shift), int(chunk_pairs), _arg(pd_q), _arg(union_q), ctypes.byref(used),
                                       _arg(d), _arg(h), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return pd_q, union_q, int(used.value), d, h

    def unifrac_null_host(self, root, univ, sets, begin=0, count=None, shift=None, permutations=0, seed=0, stream=0, chunk_tasks=0, pd=True,
                          union=True):
        """st_unifrac_null_host: (pd_q (n_sets, permutations + 1), union_q (count, permutations + 1), shift) of the position
        sets ``sets`` (as in ``dispersion_matrix``) over the universe ``univ`` (leaf ids of this tree under ``root``,
        depth-first) under every permutation of the taxa-labels null; column 0 is ``unifrac_host``.  ``pd`` / ``union``
        False: that output is not computed and comes back as None."""
        univ = np.ascontiguousarray(univ, dtype=np.int64)
        if univ.ndim != 1:
            raise ValueError("the universe must be 1-D")
        n = len(univ)
        _dispersion_args(permutations, stream, chunk_tasks)
        pos, off, n_sets = _dispersion_sets(sets, n)
        begin, count = _unifrac_range(n_sets, begin, count, 0)
        R = int(permutations) + 1
        pd_q = np.zeros((n_sets, R), dtype=np.int64) if pd else None
        union_q = np.zeros((count, R), dtype=np.int64) if union else None
        used, bad = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self._lib.st_unifrac_null_host(self.handle, int(root), _arg(univ), n, _arg(pos), len(pos), _ptr(off), n_sets, begin, count,
                                            -1 if shift is None else int(shift), int(permutations), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                            int(stream), int(chunk_tasks), _ptr(pd_q), _ptr(union_q), ctypes.byref(used), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
        return pd_q, union_q, int(used.value)

    def triangle_device(self, d_ids, m, k_begin, k_count, d_out_dist=0, d_out_mrca=0, stream=0, id_stride=1):
        rc = self._lib.st_triangle_device(self.handle, ctypes.c_void_p(d_ids), int(m), int(id_stride),
                                          int(k_begin), int(k_count), ctypes.c_void_p(d_out_dist or None),
                                          ctypes.c_void_p(d_out_mrca or None), ctypes.c_void_p(stream or None))
        check(rc)

    def distances_device(self, d_pairs, n, d_out_dist=0, d_out_mrca=0, stream=0, stride0=2, stride1=1,
                         f32=False):
        """Raw device pointers (ints); enqueues on ``stream`` without synchronising.
        ``f32``: d_out_dist is a float32 buffer (the values are float32 sums)."""
        fn = self._lib.st_distances_device_f32 if f32 else self._lib.st_distances_device
        rc = fn(self.handle, ctypes.c_void_p(d_pairs), int(n), int(stride0),
                                           int(stride1), ctypes.c_void_p(d_out_dist or None),
                                           ctypes.c_void_p(d_out_mrca or None),
                                           ctypes.c_void_p(stream or None))
        check(rc)

    def distances_device_wire(self, d_pairs, n, d_out_dist=0, d_out_mrca24=0, stream=0, stride0=2, stride1=1):
        """The wire format of result slices that travel: float32 distances, MRCA ids packed as 24 bits each
        (st_distances_device_wire; trees of fewer than 2^24 nodes)."""
        check(self._lib.st_distances_device_wire(self.handle, ctypes.c_void_p(d_pairs), int(n), int(stride0), int(stride1),
                                                 ctypes.c_void_p(d_out_dist or None), ctypes.c_void_p(d_out_mrca24 or None),
                                                 ctypes.c_void_p(stream or None)))

    def unpack_mrca24_device(self, d_packed, n, d_out_mrca, stream=0):
        check(self._lib.st_unpack_mrca24_device(int(self.devices[0]), ctypes.c_void_p(d_packed), int(n), ctypes.c_void_p(d_out_mrca),
                                                ctypes.c_void_p(stream or None)))

    def probe_last_choice(self, stream=0):
        """0 / 1: the batch probe gave this handle's last probed batch to the scalar ladder / tile-sorted walk kernel; -1: none yet."""
        c = ctypes.c_int32(-1)
        check(self._lib.st_probe_last_choice(self.handle, ctypes.c_void_p(stream or None), ctypes.byref(c)))
        return int(c.value)

    def fault_check(self, stream=0):
        bad = ctypes.c_int64(0)
        rc = self._lib.st_fault_check(self.handle, ctypes.c_void_p(stream or None), ctypes.byref(bad))
        check(rc, tree_size=self.size, bad_id=int(bad.value))
