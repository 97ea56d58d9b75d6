/*
 * suchtree_hip.h -- C ABI of libsuchtree_hip.so, the MI355X (gfx950) bulk
 * patristic-distance / MRCA engine behind suchtree_amd.SuchTree.
 *
 * The reference (ryneches/SuchTree) has no FFI layer for this path: the
 * boundary is its Cython class surface and the two cdef methods behind it.
 * Each entry point below names the reference interface it stands in for
 * (paths relative to /root/reference).  Signatures are plain C: pointers and
 * sizes only, no torch / numpy types.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns ST_OK (0) or an ST_ERR_* code; the message for
 *     the calling thread's last failure is st_last_error().
 *   - node ids are the reference's ids: positions in the in-order traversal
 *     of the strictly binary tree (SuchTree/MuchTree.pyx:171-180).
 *   - pairs are int64 (n,2) views given as a base pointer and two ELEMENT
 *     strides (the reference takes any `long[:,:]` memoryview,
 *     MuchTree.pyx:913); C order is stride0=2, stride1=1.
 *   - distances come back as float64 holding the float32 value the
 *     reference accumulates (MuchTree.pyx:922,943); MRCA ids as int32.
 *   - "_host" entry points take host buffers and do the transfers; "_device"
 *     entry points take device buffers on the tree's GPU, enqueue on the
 *     caller's hipStream_t (passed as void*, NULL = default stream) and do
 *     not synchronise.
 */
#ifndef SUCHTREE_HIP_H
#define SUCHTREE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ABI version: bumped whenever an exported struct grows, or an export, option or constant goes away.  A caller built against
 * an older header must not be handed a larger st_tree_info: compare ST_API_VERSION with st_api_version() at load (the ctypes
 * binding does) and use st_tree_info_get_sized, which writes at most the bytes the caller says it has.
 *   7: st_compare_triangle_host, st_compare_pairs_host and struct st_pair_moments added; later, without a bump (additive):
 *      st_clade_plan, st_compare_clades_host, struct st_clade_segment and the ST_CLADE_* constants; then, also additive,
 *      st_compare_rows_host; then, also additive, struct st_rank_sums, st_compare_triangle_ranks_host,
 *      st_compare_pairs_ranks_host and st_spearman_host; then st_tree_info.heap_lines appended (8 bytes) with option
 *      "heap_lines" -- callers built against the shorter struct keep using st_tree_info_get_sized; then, in the same way,
 *      st_tree_info.stream_hint appended (8 bytes) with option "stream_hint"; then, also additive, struct st_quartet_table,
 *      the ST_QUARTET_* constants, st_quartet_positions, st_compare_quartets_leaves_host and st_compare_quartets_host; then, also
 *      additive, struct st_kendall_counts, ST_KENDALL_TILE, st_compare_triangle_kendall_host, st_compare_pairs_kendall_host,
 *      st_kendall_arrays_host and st_kendall_host; then, also additive, struct st_hommola_clade, ST_HOMMOLA_MAX_UNIVERSE,
 *      st_hommola_permutation and st_hommola_clades_host; then, also additive, struct st_dispersion_record,
 *      st_partner_dispersion_host and st_dispersion_matrix; then, also additive, ST_UNIFRAC_MAX_UNIVERSE,
 *      ST_UNIFRAC_LANE_MAX, st_unifrac_host, st_unifrac_depths and st_unifrac_quantise; then st_tree_info.heap_codes appended
 *      (8 bytes) with option "heap_codes", as heap_lines was; then, also additive, ST_CLADE_MATCH_MAX_LEAVES, st_clade_ranges
 *      and st_clade_match; then, also additive, st_beta_dispersion_host and st_beta_dispersion_matrix; then, also additive,
 *      st_unifrac_null_host and st_unifrac_null_depths; then, also additive, struct st_mantel_sums, struct st_mantel_moments,
 *      ST_MANTEL_SHIFT_AUTO, st_mantel_codes and st_mantel_quantise; then, also additive, ST_GROUP_MAX and
 *      st_group_sums_codes; then, also additive, struct st_parafit_sum and st_parafit_codes; then, also additive,
 *      ST_CLASS_MAX, ST_CLASS_NONE and st_class_sums_codes; then, also additive, st_swap_null_tables, st_swap_null_schedule,
 *      st_dispersion_matrix_swap and st_partner_dispersion_swap_host; then, also additive, struct st_linkage_row, the
 *      ST_LINKAGE_* constants and st_linkage_codes; then, also additive, ST_RF_MAX_LEAVES and st_rf_tasks.
 *   6 (round 6): st_api_version, st_tree_info_get_sized, st_probe_last_choice, option "ladder_sums" added; st_tree_info.reserved0
 *                is now ladder_sums, ladder_sums_max_pairs appended (8 bytes); option "tile_sort" selects nothing on records of 128 bytes and more (kernel forms removed).
 *   5 (round 5): st_tree_info grew by 8 bytes (b_table_bytes_per_leaf, reserved0); st_host_alloc / st_host_free,
 *                ST_KERNEL_CANOPY_SCALAR, the options pairs_per_lane and ladder_dynamic = 2 removed.
 */
#define ST_API_VERSION 7
int st_api_version(void);

#define ST_OK          0
#define ST_ERR_ARG     1   /* bad argument (NULL, negative size, bad strategy) */
#define ST_ERR_HIP     2   /* a HIP runtime call failed / no usable GPU */
#define ST_ERR_BOUNDS  3   /* a node id in `pairs` is outside [0, n_nodes) */
#define ST_ERR_NOMEM   4   /* host allocation failed */
#define ST_ERR_TREE    5   /* parent array is not a single rooted binary tree */
#define ST_ERR_MEASURE_ONLY 6   /* the handle's "measure" option made this host-path call skip work: timing only, results invalid */

/* kernel families (st_tree_create `strategy`, st_tree_info.strategy) */
#define ST_STRATEGY_AUTO    0  /* canopy when the tree admits it, else walk */
#define ST_STRATEGY_WALK    1  /* pointer chase over the {parent,dist} table */
#define ST_STRATEGY_CANOPY  2  /* top of tree in LDS + per-node understory records */

typedef struct st_tree st_tree;   /* opaque: device-resident tree */

typedef struct st_tree_info {
    int64_t n_nodes;
    int64_t n_leaves;
    int32_t root;
    int32_t depth;            /* nodes on the longest leaf->root path (MuchTree.pyx:218-225) */
    int32_t device;
    int32_t strategy;         /* ST_STRATEGY_WALK or ST_STRATEGY_CANOPY actually in use */
    int32_t canopy_nodes;     /* nodes staged in LDS (0 for walk) */
    int32_t understory_max;   /* longest chain below the canopy, in nodes */
    int32_t record_bytes;     /* stride of one understory record */
    int32_t n_devices;        /* GPUs holding a replica (1 unless st_tree_create_multi) */
    int64_t device_bytes;     /* HBM held by this tree */
    int64_t lineage_entries;  /* float32 entries of the lineage-sum table (deep canopies, in-order ids), else 0 */
    int32_t big_batch_kernel; /* kernel of large distance batches: ST_KERNEL_* below */
    int32_t tuned;            /* 1 = that kernel was chosen by timing the candidates when the tree was created, 2 = read
                                 from the record an earlier handle of the same tree on the same device left, 0 = by rule */
    int32_t host_wire_bytes_in;   /* bytes per pair the st_*_host entry points ship over the link: ids in (6 or 8) ... */
    int32_t host_wire_bytes_out;  /* ... float32 distance + MRCA id back (7 or 8); follow the wire48 / wire24 options */
    int32_t a_side_bytes;     /* canopy family: bytes gathered for the first node of a pair, 4 (rec_a4 + block table) or 8 */
    int32_t dropped_tables;   /* ST_TABLE_* bits: what the table budget left out (slower forms of the kernels take over) */
    int64_t table_budget_bytes;   /* the budget this handle was built under (0 = none) */
    int32_t b_table_bytes_per_leaf;   /* canopy family: bytes per leaf of the table the second node of a leaf pair gathers from:
                                         record_bytes / 2, or record_bytes / 4 where sibling leaves share a cherry record */
    int32_t ladder_sums;      /* (was reserved0 until version 6) 1 = the scalar ladder kernel reads the first node's whole side from the
                                 lineage sums (option "ladder_sums", set by timing when a deep tree is created), 0 = it climbs both sides */
    int64_t ladder_sums_max_pairs;   /* largest batch the joint form takes when ladder_sums is 1; 0 = every batch (ml.tree: 2^20 -- beyond it the
                                        climbing form runs) */
    int64_t heap_lines;       /* 1 = explicit pair batches with distances currently take the heap-line form of the predicated kernel
                                 (perfect trees; option "heap_lines"): both nodes of a pair gather from one table of 8 bytes per
                                 leaf, so a_side_bytes and b_table_bytes_per_leaf are 4 and 4 while it is set; else 0 */
    int64_t stream_hint;      /* 1 = large explicit pair batches with distances from and to device buffers (st_distances_device*) currently
                                 read their pairs and write their results with the non-temporal hint (option "stream_hint"); else 0 */
    int64_t heap_codes;       /* 1 = large ones of those batches currently take the heap-code form of that kernel (option "heap_codes"): the same edges as
                                 20-bit codes, 24 leaves per 128-byte line.  heap_lines, a_side_bytes, b_table_bytes_per_leaf and
                                 stream_hint report what they report without it; else 0 */
} st_tree_info;

/* st_tree_info.dropped_tables, in the order in which a table budget (st_tree_options.table_budget_bytes, else
 * SUCHTREE_AMD_TABLE_MB) drops them -- every one is an accelerator, results are the same bits without it: */
#define ST_TABLE_LINEAGE_LEN   1   /* lineage lengths + crown tables: the walk family climbs b's side instead of streaming it */
#define ST_TABLE_LINEAGE_SUM   2   /* lineage sums: a's side is climbed, the tile-sorted kernels lose their lineage-sum form */
#define ST_TABLE_TREE_RMQ      4   /* whole-tree sparse table: the walk family finds meeting nodes by climbing */
#define ST_TABLE_REC_I         8   /* id chains of the understory records (as large as the b-side records: judged when the
                                      records are sized): pairs under one portal are walked on the tree */
#define ST_TABLE_REC_A4       16   /* four-byte a side of the predicated kernel and the cherry records of its b side: the 8-byte entries and rec_b serve */
#define ST_TABLE_RANKS        32   /* rank table of MRCA-only requests: they go through the distance kernels */
#define ST_TABLE_CANOPY       64   /* every canopy table: the walk family serves the tree */

/* Creation options (st_tree_create_ex); zero-initialise, then set what is wanted. */
typedef struct st_tree_options {
    int64_t table_budget_bytes;   /* device bytes the tree's tables may take; 0 = SUCHTREE_AMD_TABLE_MB (MiB) if set, else no
                                     limit.  Below the floor (28 bytes per node: parent/distance, depth and the three-level
                                     image the walk kernel needs) the floor is what is uploaded. */
    int64_t reserved[7];
} st_tree_options;

/* st_tree_info.big_batch_kernel */
#define ST_KERNEL_WALK            0   /* k_walk / k_walk_sorted: trees the canopy family does not serve */
#define ST_KERNEL_CANOPY          1   /* predicated canopy kernel (one pair per lane, chain in registers); 2: unused since round 5 */
#define ST_KERNEL_CANOPY_SORTED   3   /* tile-sorted canopy kernel (ladder form of the canopy in LDS; chains of at most seven slots) */
#define ST_KERNEL_WALK_SORTED     4   /* tile-sorted walk kernel on a tree that also has canopy tables */
#define ST_KERNEL_CANOPY_LADDER   5   /* scalar canopy kernel over the ladder form (long records in registers, read once) */

/* Last error message of the calling thread ("" if none). */
const char *st_last_error(void);

/* Number of visible HIP devices. */
int st_device_count(int *count);

/*
 * Upload a tree.  Replaces the reference's in-object `Node* data` filled at
 * SuchTree/MuchTree.pyx:158-216 (parent / distance columns) and the `depth`
 * scan at :218-225.  `parent[root] == -1`; `distance` are the float32 branch
 * lengths exactly as the reference stores them (root entry ignored).
 * All derived tables (depths, canopy, understory records) are built here,
 * once, and stay resident in HBM until st_tree_destroy.
 */
int st_tree_create(const int32_t *parent, const float *distance, int64_t n_nodes,
                   int device, int strategy, st_tree **out);

/*
 * Same tree replicated on several GPUs of one node, driven from ONE process: the reference's
 * user calls T.distances(ids) from a single process (SuchTree/MuchTree.pyx:872-909) and
 * parallelises with a fork pool over contiguous chunks
 * (docs/examples/SuchTree_examples.md:462-497); here the "_host" entry points deal their
 * pipeline chunks round-robin over `devices` (one host thread, one staging pipe and one
 * PCIe link per GPU; st_host_chunk_plan / st_host_chunk_owner state the map).  The tables
 * are built once and uploaded to every listed device.  Device-pointer entry points, the
 * small-batch mailbox and st_quartets_host use devices[0].
 */
int st_tree_create_multi(const int32_t *parent, const float *distance, int64_t n_nodes,
                         const int *devices, int n_devices, int strategy, st_tree **out);

/*
 * The same with creation options: a budget for the device tables.  A tree costs 28 bytes per node on the device (the
 * floor); everything beyond that -- 60 to 1500 times the reference's 20-byte Node -- is accelerator tables, and under
 * a budget they are left out in the order of the ST_TABLE_* bits above until the rest fits; st_tree_info reports
 * device_bytes and dropped_tables.  opts may be NULL (= st_tree_create_multi).  No counterpart in the reference,
 * whose tree is one calloc of n nodes (SuchTree/MuchTree.pyx:114, 160-165).
 */
int st_tree_create_ex(const int32_t *parent, const float *distance, int64_t n_nodes,
                      const int *devices, int n_devices, int strategy, const st_tree_options *opts, st_tree **out);

/* Host-only helper, no GPU needed: what st_tree_create_ex would build for this tree under `table_budget_bytes`
 * (0 = SUCHTREE_AMD_TABLE_MB if set, else no limit): the device bytes, the ST_TABLE_* bits left out and the family. */
int st_host_table_plan(const int32_t *parent, const float *distance, int64_t n_nodes, int strategy,
                       int64_t table_budget_bytes, int64_t *device_bytes, int32_t *dropped_tables, int32_t *family);

/* Devices of a handle, devices[0] first (devices may be NULL to ask for the count only). */
int st_tree_devices(const st_tree *tree, int *devices, int capacity, int *n_devices);

/*
 * How a host batch of n pairs is cut into pipeline chunks and which device of a
 * multi-device handle gets which chunk (no GPU needed): chunk c covers
 * [c * chunk_pairs, min(n, (c+1) * chunk_pairs)) and is computed by devices[c % n_devices].
 */
int st_host_chunk_plan(int64_t n, int n_devices, int64_t *chunk_pairs, int64_t *n_chunks);
int st_host_chunk_owner(int64_t n, int n_devices, int64_t chunk_index, int *device_index,
                        int64_t *first_pair, int64_t *n_pairs);

/* Replaces SuchTree.__dealloc__ (MuchTree.pyx:230-232). */
void st_tree_destroy(st_tree *tree);

/* Fills *info (sizeof(st_tree_info) bytes of THIS header's struct: callers compiled against it only). */
int st_tree_info_get(const st_tree *tree, st_tree_info *info);
/* The same for a caller that states how large ITS st_tree_info is: at most info_bytes bytes are written (fields are only ever
 * appended, so a shorter struct is a prefix); info_bytes < 8 or not a multiple of 4 is ST_ERR_ARG. */
int st_tree_info_get_sized(const st_tree *tree, void *info, int64_t info_bytes);

/*
 * Bulk distances (+ MRCA ids) for host-resident pairs.  Replaces
 * SuchTree._distances (SuchTree/MuchTree.pyx:911-943, which calls _mrca
 * :999-1030) as invoked by distances_bulk (:872-909).
 * out_dist and out_mrca may each be NULL (not both).  On ST_ERR_BOUNDS
 * *bad_id (if non-NULL) receives the id the reference would report
 * (max id if it is >= n_nodes, else the min id; MuchTree.pyx:897-903) and the
 * outputs are unspecified.
 */
int st_distances_host(st_tree *tree, const int64_t *pairs, int64_t n,
                      int64_t stride0, int64_t stride1,
                      double *out_dist, int32_t *out_mrca, int64_t *bad_id);

/* Same for int32 ids (element strides of the int32 view): half the host-side read traffic,
 * and a C-order array is already what is sent over PCIe. */
int st_distances_host_i32(st_tree *tree, const int32_t *pairs, int64_t n,
                          int64_t stride0, int64_t stride1,
                          double *out_dist, int32_t *out_mrca, int64_t *bad_id);

/*
 * Same computation on device-resident buffers, enqueued on `stream`
 * (a hipStream_t; NULL = default stream).  Does not synchronise.  Out-of-range
 * ids never dereference the tree: such pairs produce NaN / -1 and are
 * recorded in the tree's device-path fault word, read back by st_fault_check
 * (the "_host" entry points keep a fault word of their own).
 */
int st_distances_device(st_tree *tree, const int64_t *d_pairs, int64_t n,
                        int64_t stride0, int64_t stride1,
                        double *d_out_dist, int32_t *d_out_mrca, void *stream);

/* Same, writing the distances as the float32 values they are (half the output bytes; the
 * float64 form above holds exactly these values widened). */
int st_distances_device_f32(st_tree *tree, const int64_t *d_pairs, int64_t n,
                            int64_t stride0, int64_t stride1,
                            float *d_out_dist, int32_t *d_out_mrca, void *stream);

/*
 * Wire format of result slices that travel (multi-GPU gather over xGMI, suchtree_amd/sharding.py::run_sharded;
 * the host path ships the same format over PCIe): float32 distances and MRCA ids as 24 bits each -- id i at bytes
 * [3 i, 3 i + 3) of d_out_mrca24, little endian, -1 (an id out of range) as 0xFFFFFF -- 7 bytes per pair instead of
 * the 12 of float64 + int32.  The kernels assemble the packed stream themselves (no packing pass).  Trees of fewer
 * than 2^24 nodes only (ST_ERR_ARG otherwise); d_out_mrca24 must be 4-byte aligned and hold 3 n bytes rounded up to
 * a multiple of 4 (the last dword is written whole).  Either output may be NULL.  No counterpart in the reference,
 * whose only parallel recipe is a fork pool (docs/examples/SuchTree_examples.md:462-497).
 */
int st_distances_device_wire(st_tree *tree, const int64_t *d_pairs, int64_t n,
                             int64_t stride0, int64_t stride1,
                             float *d_out_dist, uint8_t *d_out_mrca24, void *stream);

/* The receiving side: n packed 24-bit ids at d_packed (any byte alignment) -> int32 at d_out_mrca (0xFFFFFF -> -1),
 * enqueued on `stream` of `device`. */
int st_unpack_mrca24_device(int device, const uint8_t *d_packed, int64_t n, int32_t *d_out_mrca, void *stream);

/*
 * Synchronise `stream`, then report and clear the fault word written by
 * earlier st_distances_device calls: ST_OK, or ST_ERR_BOUNDS with *bad_id set
 * as for st_distances_host.
 */
int st_fault_check(st_tree *tree, void *stream, int64_t *bad_id);

/*
 * Diagnostic: which kernel the batch probe gave the handle's most recent probed batch (large device-resident batches of
 * explicit pairs on deep trees decide per batch, on the device: option batch_probe).  Synchronises `stream`.
 * *choice = 0 scalar ladder kernel, 1 tile-sorted walk kernel, -1 no batch of this handle has been probed yet.
 */
int st_probe_last_choice(st_tree *tree, void *stream, int *choice);

/*
 * All-pairs generator: for an id list ids[0..m) (element stride id_stride) computes
 * pair k = (ids[j], ids[i]), k = i(i-1)/2 + j, 0 <= j < i < m, for k in
 * [k_begin, k_begin + k_count); out[k - k_begin] receives the result.  No pair array
 * exists anywhere: the kernel derives (i, j) from k.  Replaces the nested pair loops of
 * SuchLinkedTrees.linked_distances (SuchTree/MuchTree.pyx:2918-2925, ids = a linklist
 * column) and, up to enumeration order, of SuchTree.pairwise_distances (:1106-1114),
 * followed by _distances (:911-943).  The k-range lets callers shard the triangle by
 * equal pair counts across GPUs and stream it in tiles.
 */
int st_triangle_device(st_tree *tree, const int64_t *d_ids, int64_t m, int64_t id_stride,
                       int64_t k_begin, int64_t k_count,
                       double *d_out_dist, int32_t *d_out_mrca, void *stream);
int st_triangle_host(st_tree *tree, const int64_t *ids, int64_t m, int64_t id_stride,
                     int64_t k_begin, int64_t k_count,
                     double *out_dist, int32_t *out_mrca, int64_t *bad_id);

/*
 * Grid generator: for id lists row_ids[0..n_rows) and col_ids[0..n_cols) (contiguous int64)
 * computes element e = r * n_cols + c, the pair (row_ids[r], col_ids[c]), for e in
 * [e_begin, e_begin + e_count); out[e - e_begin] receives the result.  With `symmetric` != 0
 * (same list on both sides) elements below the diagonal take their mirror image's argument
 * order, so the whole range [0, n^2) IS the symmetric matrix of SuchTree.pairwise_distances
 * (SuchTree/MuchTree.pyx:1084-1124: pairs (ids[i], ids[j]), i < j, scattered to [i,j] and
 * [j,i]; zero diagonal), written straight into the caller's (n,n) float64 array -- the
 * reference's Python pair list and its scatter loop (:1106-1122) have no counterpart.
 * A rectangular grid is the distance block of nearest_neighbors (:1069-1072).
 */
int st_grid_host(st_tree *tree, const int64_t *row_ids, int64_t n_rows,
                 const int64_t *col_ids, int64_t n_cols, int symmetric,
                 int64_t e_begin, int64_t e_count,
                 double *out_dist, int32_t *out_mrca, int64_t *bad_id);

/*
 * k nearest candidates of every query: distances query -> cands on the device, then a
 * per-row selection of the k smallest (ties: lower candidate index first), both on the GPU.
 * Replaces the pair list, distances_bulk call and np.argsort of SuchTree.nearest_neighbors
 * (SuchTree/MuchTree.pyx:1069-1082) for many queries at once.  out_index (n_queries, k) holds
 * positions in `cands` (-1 where fewer than k candidates exist), out_dist (n_queries, k) the
 * distances, ascending.  skip_self != 0 ignores candidates equal to the query id (the
 * reference drops a leaf query from its default candidate list, :1058-1062).  1 <= k <= 256.
 */
int st_knn_host(st_tree *tree, const int64_t *queries, int64_t n_queries,
                const int64_t *cands, int64_t n_cands, int k, int skip_self,
                int64_t *out_index, double *out_dist, int64_t *bad_id);

/*
 * Compare two trees' distances over the same pairs, reduced on the GPU.  Pair k is evaluated in tree_x (x_k) and in
 * tree_y (y_k) by the same kernels as the calls above (float32 sums, bit-identical to st_distances_host / st_triangle_host);
 * out receives the moments of the joint distribution and, if edges_x, edges_y and out_hist are all given, out_hist the
 * exact 2-D histogram of numpy.histogram2d on the float64-widened values: cell (i, j) of the C-order int64
 * (bins_x, bins_y) array counts the pairs with x in bin i and y in bin j, bin = searchsorted(edges, v, side='right') - 1,
 * a value equal to the last edge in the last bin, values outside [edges[0], edges[bins]] and NaN not counted.  Edges:
 * bins + 1 finite, monotonically increasing doubles per axis, first < last; at most 16384 cells.  Nothing is returned
 * per pair: device scratch is bounded by a chunk of pairs, host memory by the histogram.
 *
 * Replaces the host-side reduction of the reference's two comparison workflows: docs/examples/SuchTree_examples.md
 * ("Comparing the topologies of two large trees") and docs/benchmarks.md, which draw random name pairs, call
 * distances_by_name (SuchTree/MuchTree.pyx:945-979) on both trees and correlate the two lists; and
 * SuchLinkedTrees.linked_distances (SuchTree/MuchTree.pyx:2900-2934), whose two columns every notebook correlates
 * (sample_linked_distances, :2951-3079, samples them because the pairs are too many to enumerate on a CPU).
 *
 * Both trees must live on the same device (a multi-device handle: its first device), otherwise ST_ERR_ARG; tree_x ==
 * tree_y is allowed.  Ids are checked on the host before anything is launched: ST_ERR_BOUNDS with *bad_id as for
 * st_distances_host (tree_x's ids first).  Bad histogram arguments -- some but not all of edges_x / edges_y / out_hist
 * NULL, a bins < 1, more than 16384 cells, edges not increasing -- are ST_ERR_ARG.
 *
 * The sums are taken about a shift (cx, cy), the mean of the call's first min(count, 4096) pairs (0 where that mean is
 * not finite), against cancellation; they are reduced in one fixed order (lanes, waves, workgroups of a fixed grid,
 * then the workgroups in index order, no float atomics): two identical calls return identical bits.  NaN distances
 * propagate into the sums and are skipped by min / max and the histogram.  An empty range gives n = 0, zero sums,
 * NaN min / max and a zero histogram, and launches nothing.  No counterpart in the reference.
 */
typedef struct st_pair_moments {
    int64_t n;                        /* pairs reduced */
    double  shift_x, shift_y;         /* cx, cy used for the sums below */
    double  sx, sy, sxx, syy, sxy;    /* sums of (x-cx), (y-cy), squares, cross product */
    double  min_x, max_x, min_y, max_y;
} st_pair_moments;

/* pair k = (ids_x[j], ids_x[i]) in tree_x and (ids_y[j], ids_y[i]) in tree_y, k = i(i-1)/2 + j, for k in
   [k_begin, k_begin + k_count) -- the enumeration of st_triangle_host.  edges_* / out_hist may be NULL (no histogram). */
int st_compare_triangle_host(st_tree *tree_x, st_tree *tree_y, const int64_t *ids_x, const int64_t *ids_y, int64_t m,
                             int64_t k_begin, int64_t k_count,
                             const double *edges_x, int32_t bins_x, const double *edges_y, int32_t bins_y,
                             st_pair_moments *out, int64_t *out_hist, int64_t *bad_id);
/* pair i = (pairs_x[i,0], pairs_x[i,1]) in tree_x and (pairs_y[i,0], pairs_y[i,1]) in tree_y; C-order int64 (n,2). */
int st_compare_pairs_host(st_tree *tree_x, st_tree *tree_y, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n,
                          const double *edges_x, int32_t bins_x, const double *edges_y, int32_t bins_y,
                          st_pair_moments *out, int64_t *out_hist, int64_t *bad_id);

/*
 * Every clade at once: the moments of linked distances of every node of a clade tree (tree_y), in one pass over the pairs.
 * Links j = 0 .. n_links-1 are given in rank order: link j is leaf ids_y[j] of the clade tree and node ids_x[j] of
 * tree_x.  The pairs of node v are the pairs of links whose clade-side leaves both lie under v, each evaluated as
 * (lower rank, higher rank) in both trees -- the orientation of st_compare_triangle_host over the links under v in rank
 * order, so every node's per-pair values are bit-identical to that call's.
 *
 * The pairs are cut into segments (st_clade_plan): links are permuted so that every node's links are one contiguous
 * range; a rectangle of node v holds the pairs between one child's links and the links of v's later children, a
 * triangle of leaf l the pairs of the links that share l.  Every pair lies in exactly one segment; a node's pairs are
 * the segments of its subtree.  With max_links >= 0 only nodes with at most max_links links get their segments.
 *
 * Parent arrays: int32, n_nodes entries, -1 at the one root; children of a node are taken in increasing id order.
 * A parent array that is not one rooted tree is ST_ERR_TREE; a link leaf id outside [0, n_nodes) ST_ERR_BOUNDS with
 * *bad_id; a link leaf id that is not a leaf ST_ERR_ARG.  No counterpart in the reference.
 */
#define ST_CLADE_RECT 0       /* segment kind: rows x cols */
#define ST_CLADE_TRI  1       /* segment kind: all pairs within rows (cols unused) */
#define ST_CLADE_TILE 8192    /* pairs per tile of the clade reduction; chunk_pairs must be a multiple of it */
typedef struct st_clade_segment {
    int64_t first_pair;            /* global index k of its first pair */
    int64_t n_pairs;
    int32_t kind;                  /* ST_CLADE_RECT / ST_CLADE_TRI */
    int32_t node;                  /* the node (rectangle) or leaf (triangle) whose pairs these are */
    int32_t row_begin, row_end;    /* positions in the permuted link order */
    int32_t col_begin, col_end;
} st_clade_segment;

/* Host only.  out_perm[p] = rank of the link at position p (n_links entries); out_begin / out_count (n_nodes each):
 * node v's links are positions [out_begin[v], out_begin[v] + out_count[v]); out_leaves (n_nodes, may be NULL): leaves
 * under v.  out_segs (room for seg_capacity >= 2 n_nodes entries, may be NULL to count only) receives the non-empty
 * segments in pair order, *out_n_segs their number and *out_total_pairs the pairs they hold. */
int st_clade_plan(const int32_t *parent, int64_t n_nodes, const int64_t *link_leaf, int64_t n_links, int64_t max_links,
                  int64_t *out_perm, int64_t *out_begin, int64_t *out_count, int64_t *out_leaves,
                  st_clade_segment *out_segs, int64_t seg_capacity, int64_t *out_n_segs, int64_t *out_total_pairs,
                  int64_t *bad_id);
/* out (n_nodes entries): node v's moments; n = -1 and NaN elsewhere for a node with more than max_links links (not
 * computed; max_links < 0: no cap), n = 0 with zero sums and NaN min / max for a node with fewer than two.  out_count
 * (n_nodes, may be NULL): links under each node.  n_nodes must be tree_y's node count.  chunk_pairs: pairs per device
 * chunk, 0 = the default, else a positive multiple of ST_CLADE_TILE.  Trees and ids as for st_compare_triangle_host.
 * Each tile-sized piece of a segment is summed about its own first pair in one fixed order, pieces are merged into
 * segments and segments into nodes (children first, in increasing id order, then the node's own segments) with the
 * shifted pairwise update on the host: results do not depend on the device, the grid or chunk_pairs. */
int st_compare_clades_host(st_tree *tree_x, st_tree *tree_y, const int32_t *parent, int64_t n_nodes, const int64_t *ids_x,
                           const int64_t *ids_y, int64_t n_links, int64_t max_links, int64_t chunk_pairs,
                           st_pair_moments *out, int64_t *out_count, int64_t *bad_id);

/*
 * Many triangles in one pass: row r of the C-order int64 (n_rows, m) arrays ids_x / ids_y is one
 * st_compare_triangle_host over all of its pairs -- pair k = (ids_x[r,j], ids_x[r,i]) in tree_x and (ids_y[r,j],
 * ids_y[r,i]) in tree_y, k = i(i-1)/2 + j -- and out[r] (n_rows entries) receives that row's moments, summed about the
 * row's first pair (0 where it is not finite).  A row with m < 2 gives n = 0, zero sums and NaN min / max.  The rows of
 * a permutation test (SuchLinkedTrees.hommola_cospeciation: the links relabelled once per permutation) are such rows.
 * Trees, ids and error codes as for st_compare_triangle_host; chunk_pairs: 0 (the default) or a positive multiple of
 * ST_CLADE_TILE, else ST_ERR_ARG.  Device memory is bounded by one chunk of pairs, the ids of its rows and its blocks.
 *
 * Determinism: out[r] depends only on row r's ids and the two trees -- not on r, the other rows, n_rows, chunk_pairs
 * or the device.  A row is cut into blocks of ST_CLADE_TILE pairs counted from its first pair; each block is summed
 * about its own first pair in one fixed order that depends on its length alone, and the blocks are merged in block
 * order with the shifted pairwise update (the operation order of DistanceComparison.merge).  Identical rows give
 * identical bits wherever they stand.  No float atomics.  No counterpart in the reference.
 */
int st_compare_rows_host(st_tree *tree_x, st_tree *tree_y, const int64_t *ids_x, const int64_t *ids_y,
                         int64_t n_rows, int64_t m, int64_t chunk_pairs,
                         st_pair_moments *out, int64_t *bad_id);

/*
 * Hommola's permutation test of cospeciation for many clades of one tree in one pass (SuchLinkedTrees.hommola_by_clade).
 * tree_c is the clade tree, tree_o the other tree; x = tree_o, y = tree_c.
 *
 * Orders.  univ_c (n_univ_c ids) are the clade tree's leaves in an order in which every clade is one range
 * [leaf_begin, leaf_begin + leaf_count) -- depth-first, children in increasing id order -- and univ_o (n_univ_o ids) the
 * other tree's leaves.  Link l (0 <= l < n_links) joins position pos_o[l] of univ_o and pos_c[l] of univ_c; the links are
 * laid out so that pos_c is non-decreasing (the order of st_clade_plan's out_perm), hence every clade's links are one
 * range [link_begin, link_begin + link_count).  Pair t = i(i-1)/2 + j (j < i) of a clade of L links is (link j, link i)
 * of its range, with x = D_o[q_o(j)][q_o(i)] and y = D_c[q_c(j)][q_c(i)], D[p][q] = dist(u[p], u[q]) with the arguments in
 * that order (both triangles are kept: the float32 sums are not symmetric in the last bit) and q the link's position,
 * relabelled.
 *
 * Permutations.  Row p = 0 of a clade is the identity; row p >= 1 relabels a link at position i to sigma[i], on the
 * clade side over the clade's own range (offset by leaf_begin) with side s = 0, on the other side over all of univ_o
 * with s = 1.  For (seed, clade node id c, p, s, universe size n), with mix the splitmix64 finalizer of
 * ST_QUARTET_SAMPLE, G = 0x9E3779B97F4A7C15 and all arithmetic mod 2^64:
 *     h0 = mix(seed + (c + 1) G),  h1 = mix(h0 + (2p + s) G),
 *     w_i = (mix(h1 + (i + 1) G) & 0xFFFFFFFFFFFF0000) | i  for i = 0 .. n-1,
 *     sigma[j] = the low 16 bits of the j-th smallest w.
 * The w are distinct, so sigma does not depend on the sorting method; universes therefore hold at most
 * ST_HOMMOLA_MAX_UNIVERSE positions.  A clade's rows depend on (seed, c, its links, the two universes) alone -- not on the
 * other clades, on chunk_blocks or on the device -- and row p is the same whatever `permutations` >= p.
 *
 * Sums.  out holds n_clades x (permutations + 1) records, row p of clade k at out[k * (permutations + 1) + p].  A row is
 * cut into blocks of ST_CLADE_TILE pairs from its first pair, each block is summed about its own first pair by the order
 * rule of st_compare_rows_host and the blocks are merged in block order: every record is bit-identical to
 * st_compare_rows_host on the relabelled ids u_o[q_o], u_c[q_c].  A clade of fewer than two links gives n = 0, zero sums
 * and NaN min / max.  No float atomics.
 *
 * Conventions and error order as for st_compare_rows_host: both trees on one device; the universe ids are checked on the
 * host before anything is launched (ST_ERR_BOUNDS with *bad_id, tree_o's ids first).  ST_ERR_ARG: pos_c not
 * non-decreasing, a position outside its universe, a clade whose link range is not exactly the links inside its leaf
 * range, clade ranges that are not laminar (nested or disjoint), a universe above the limit, a negative permutations
 * or chunk_blocks.  chunk_blocks: blocks per device chunk, 0 = the default; the result does not depend on it.  Zero
 * clades or zero links launch nothing.  Device memory: 4 (n_univ_o^2 + the sum over the maximal clade ranges of
 * leaf_count^2) bytes of matrices, the ids and positions, and one chunk of positions and pieces; an allocation that
 * fails is ST_ERR_NOMEM with the bytes asked for.  No counterpart in the reference, whose SuchLinkedTrees notebook loops
 * subset_b over the clades and takes the parametric p of scipy.stats.pearsonr.
 */
#define ST_HOMMOLA_MAX_UNIVERSE 16384
typedef struct st_hommola_clade {
    int32_t node;                      /* the clade's node id: seeds its permutations */
    int32_t leaf_begin, leaf_count;    /* its leaves: positions of univ_c */
    int32_t link_begin, link_count;    /* its links */
    int32_t reserved;
} st_hommola_clade;

/* The permutation sigma of (seed, node, p, side) over n positions as int32, 1 <= n <= ST_HOMMOLA_MAX_UNIVERSE (p = 0: the
 * identity).  device = -1 computes it on the host (no GPU); device >= 0 runs the sort of the relabelling kernel there and
 * copies its output back: the same values.  A bad n, p, side or node is ST_ERR_ARG.  No counterpart in the reference. */
int st_hommola_permutation(int device, uint64_t seed, int32_t node, int64_t p, int side, int32_t n, int32_t *out);

int st_hommola_clades_host(st_tree *tree_o, st_tree *tree_c, const int64_t *univ_o, int32_t n_univ_o, const int64_t *univ_c,
                           int32_t n_univ_c, const int32_t *pos_o, const int32_t *pos_c, int64_t n_links,
                           const st_hommola_clade *clades, int64_t n_clades, int64_t permutations, uint64_t seed,
                           int64_t chunk_blocks, st_pair_moments *out, int64_t *bad_id);

/*
 * How closely related are the members of a set of leaves: the sums behind MPD (mean pairwise distance) and MNTD (mean
 * distance to the nearest other member) of many sets over one universe, each with the null that shuffles the universe's
 * labels (picante's ses.mpd / ses.mntd with null.model = "taxa.labels").  SuchLinkedTrees.partner_dispersion asks it of
 * every leaf's partners in the other tree; SuchTree.dispersion of any sets of leaves.
 *
 * Universe and matrix.  univ (n_univ ids, 3 <= n_univ <= ST_HOMMOLA_MAX_UNIVERSE) are leaves of the tree in depth-first
 * order, children in increasing id order (the order of st_hommola_clades_host).  D[a][b] = dist(u[a], u[b]) as float32,
 * the arguments in that order; both triangles are kept (the float32 sums are not symmetric in the last bit).  It is
 * written once by the distance kernels.
 *
 * Sets.  Set r (0 <= r < n_sets) is the k_r = sets[r + 1] - sets[r] positions set_pos[sets[r] .. sets[r + 1]) of the
 * universe, strictly increasing: s_0 < s_1 < ... < s_{k-1}.  sets holds n_sets + 1 offsets, 0 <= sets[r] <= sets[r + 1]
 * <= n_pos (sets may share positions of set_pos).
 *
 * Relabelling.  Under permutation p the set is relabelled to q_i = sigma_p[s_i], sigma_p = st_hommola_permutation(seed,
 * node = stream, p, side = 0, n_univ): p = 0 is the identity, `stream` any non-negative int32 (the facade passes the
 * universe's subset root).  One sigma_p serves every set of the call, as the taxa-labels null is defined: a set's null
 * draws are uniform k-subsets of the universe, and the sets of a call share the shuffles.
 *
 * Record.  out holds n_sets x (permutations + 1) records, (r, p) at out[r * (permutations + 1) + p]:
 *     rowsum_i = sum over j != i of (double) D[q_i][q_j], added one by one with j ascending, from 0.0;
 *     rowmin_i = m after: m = +inf; for j != i ascending: v = D[q_i][q_j]; m = v < m ? v : m
 *                (a NaN entry is never taken; of equal values, -0.0 and +0.0 among them, the first stays);
 *     pair_sum = sum over i of rowsum_i,  nearest_sum = sum over i of (double) rowmin_i.
 * The caller forms MPD = pair_sum / (k (k - 1)) and MNTD = nearest_sum / k.  k < 2 gives a record of zeros.
 * The order over i depends on k alone:
 *     k <= 64: element i sits in lane i of K' lanes, K' = max(2, the next power of two >= k), the other lanes hold +0.0,
 *              and `a += a of lane (l xor o)` runs over o = K'/2, K'/4 .. 1; every lane ends with the total.
 *     k > 64:  256 lanes; lane t adds its elements i = t, t + 256, ... in ascending order from 0.0; each of the four
 *              waves of 64 lanes runs the butterfly o = 32 .. 1; then total = ((w0 + w1) + w2) + w3.
 * Record (r, p) depends on (seed, stream, p, D, set r) alone -- not on r, the other sets, permutations, chunk_tasks, the
 * grid or the device; identical sets give identical bits wherever they stand; column p is the same for any permutations
 * >= p.  No float atomics.
 *
 * st_partner_dispersion_host builds D on the tree's device (4 n_univ^2 bytes) and runs the kernels.  The universe ids are
 * checked on the host before anything is launched (ST_ERR_BOUNDS with *bad_id).  ST_ERR_ARG: a universe size outside
 * 3 .. ST_HOMMOLA_MAX_UNIVERSE, bad offsets, a position outside the universe, a set that is not strictly increasing,
 * negative permutations, chunk_tasks or stream.  chunk_tasks: (set, permutation) tasks per device chunk, and the most
 * permutations whose sigma the device holds at once; 0 = the default; the result does not depend on it.  An allocation
 * that fails is ST_ERR_NOMEM with the bytes asked for, before out is written.  Zero sets, or none of two positions,
 * launch nothing.
 *
 * st_dispersion_matrix is the same reduction over the caller's C-order float32 n x n matrix D: device = -1 computes it on
 * the host, operation for operation (no GPU); device >= 0 uploads D and runs the same kernels: the same bits.
 * No counterpart in the reference.
 */
typedef struct st_dispersion_record {
    double pair_sum, nearest_sum;
} st_dispersion_record;

int st_partner_dispersion_host(st_tree *tree, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos,
                               const int64_t *sets, int64_t n_sets, int64_t permutations, uint64_t seed, int32_t stream,
                               int64_t chunk_tasks, st_dispersion_record *out, int64_t *bad_id);

int st_dispersion_matrix(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                         int64_t n_sets, int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                         st_dispersion_record *out);

/*
 * The degree-preserving swap null of the dispersion calls (picante's "independentswap" / "trialswap", the fixed-fixed null
 * of bipartite network analysis).  The taxa-labels null above keeps every set's size and forgets how many sets a position
 * belongs to; this one keeps both margins of the 0/1 link matrix whose rows are the sets and whose columns are the
 * positions.  SuchTree.dispersion and SuchLinkedTrees.partner_dispersion take it with null = "swap".
 *
 * The chain.  Inputs are those of st_dispersion_matrix: n_univ (3 .. ST_HOMMOLA_MAX_UNIVERSE), the set table (set r is the
 * strictly increasing positions set_pos[sets[r] .. sets[r + 1])), seed, stream, and `iterations` T >= 0.  The links are the
 * L = sets[n_sets] - sets[0] entries from sets[0] on; entry e belongs to row row_of(e).  Chain p >= 1 starts from the
 * observed entries col[e] = set_pos[sets[0] + e] with h1 = perm_stream(seed, stream, p, 1) -- the stream hash of
 * st_hommola_permutation with side 1, which keeps it apart from the sigma rows (side 0) of the same stream; G =
 * 0x9E3779B97F4A7C15 and mix() are its constant and its mixer.  For t = 0 .. T - 1 in order:
 *     e1 = high 64 bits of mix(h1 + (2 t + 1) G) x L,  e2 = high 64 bits of mix(h1 + (2 t + 2) G) x L,
 *     r1 = row_of(e1), r2 = row_of(e2), b = col[e1], d = col[e2];
 *     accept iff r1 != r2 and b != d and d is not in row r1 and b is not in row r2;  on accept col[e1] = d, col[e2] = b.
 * After trial T - 1 every row is sorted ascending: that is table row p, n_pos uint16 values with the offsets of `sets`
 * (entries of set_pos outside the links are copied).  p = 0 is the observed positions; accepted[p] is the number of accepted
 * trials (0 for p = 0).  Row sums and column sums of the 0/1 matrix are the observation's for every p.  Chain p depends on
 * (seed, stream, p, T, the sets) alone -- not on n_perms, p_begin, chunk_tasks, the grid or the device.  L < 2 makes every
 * chain the observation.  The facades' default, iterations = None, is max(1000, 10 L) trials: the library's own
 * definition (picante's default is 1000 swaps).
 *
 * st_swap_null_tables writes table rows p_begin .. p_begin + n_perms to out (n_perms x n_pos uint16) and, where accepted
 * is not NULL, their accepted counts.  device = -1 is the host restatement (no GPU); device >= 0 runs k_swap_chains, one
 * wave per chain: the same values.  st_swap_null_schedule runs chain p on the host in the wave's schedule -- batches of 64
 * trials, of which the lanes below the first one that shares a row with an earlier lane are executed -- and reports the
 * batches as *steps (NULL allowed): the same row and count, by a different route.
 *
 * st_dispersion_matrix_swap and st_partner_dispersion_swap_host mirror st_dispersion_matrix and
 * st_partner_dispersion_host: record (r, p) is the record of the dispersion calls over set r of table row p -- the same
 * arithmetic, the same order over i.  Sets of fewer than two positions take part in the swaps and give zero records.
 * accepted (permutations + 1 entries) may be NULL.  device = -1 is the host restatement: the same bits.
 *
 * Errors come in the order of the calls they mirror (st_swap_null_tables: the universe size, negative p_begin, n_perms or
 * stream, the set table), then: negative iterations; a single chain whose state -- its table row and a bit matrix of
 * n_sets rows of n_univ bits padded to 64 -- exceeds the work budget of 4 GiB, ST_ERR_ARG with the bytes; then the
 * remaining checks of the mirrored call; an allocation that fails is ST_ERR_NOMEM with the bytes asked for, before out is
 * written.  Device memory: a block of chains holds 2 n_pos + 8 n_sets ceil(n_univ / 64) bytes per chain, as many chains as
 * the budget allows; chunk_tasks > 0 bounds the chains of a block as it bounds the sigma rows of st_dispersion_matrix.
 * No counterpart in the reference.
 */
int st_swap_null_tables(int device, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets,
                        int64_t p_begin, int64_t n_perms, int64_t iterations, uint64_t seed, int32_t stream, uint16_t *out,
                        int64_t *accepted);

int st_swap_null_schedule(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t p,
                          int64_t iterations, uint64_t seed, int32_t stream, uint16_t *out, int64_t *accepted, int64_t *steps);

int st_dispersion_matrix_swap(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                              int64_t n_sets, int64_t permutations, int64_t iterations, uint64_t seed, int32_t stream,
                              int64_t chunk_tasks, st_dispersion_record *out, int64_t *accepted);

int st_partner_dispersion_swap_host(st_tree *tree, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos,
                                    const int64_t *sets, int64_t n_sets, int64_t permutations, int64_t iterations, uint64_t seed,
                                    int32_t stream, int64_t chunk_tasks, st_dispersion_record *out, int64_t *accepted,
                                    int64_t *bad_id);

/*
 * How far apart are the members of two sets of leaves: the sums behind betaMPD (the mean distance between a member of one
 * set and a member of the other) and betaMNTD (the mean distance from a member to the nearest member of the other set) of
 * pairs of sets, each with the taxa-labels null of st_partner_dispersion_host (picante's comdist / comdistnt with
 * abundance.weighted = FALSE and exclude.conspecifics = exclude_shared; standardised, betaNRI and betaNTI).
 * SuchLinkedTrees.partner_beta_dispersion asks it of every two leaves' partners; SuchTree.beta_dispersion of any sets.
 *
 * The universe, D (both triangles kept), the sets, sigma_p, stream and seed are exactly those of
 * st_partner_dispersion_host; p = 0 is the identity.  Sets of 0 or 1 positions are allowed.
 *
 * Pairs.  Unordered pairs of sets (i, j), j < i, in the triangle order k = i (i - 1) / 2 + j of st_unifrac_host; a call
 * covers [begin, begin + count).
 *
 * Directions.  A pair has two: i -> j, then j -> i.  For direction r -> c under permutation p, q_a = sigma_p[s^r_a] for
 * a < k_r and q'_b = sigma_p[s^c_b] for b < k_c.  Entry (a, b) is included unless exclude_shared != 0 and s^r_a == s^c_b:
 * the comparison is on positions, so it does not depend on p.
 *     rowsum_a = sum over included b ascending of (double) D[q_a][q'_b], one by one from 0.0;
 *     rowmin_a = m after: m = +inf; for included b ascending: v = D[q_a][q'_b]; m = v < m ? v : m
 *                (the NaN and -0.0 rule of the dispersion record);
 *     an element with no included entry adds +0.0 to both sums: only when k_c == 0, or when exclude_shared is set,
 *     k_c == 1 and the single member is shared -- decided by the sets, never by the value of m;
 *     cross_sum = sum over a of rowsum_a,  nearest_sum = sum over a of (double) rowmin_a,
 * in the order over a of the dispersion record with k = k_r: k_r <= 64 the K'-lane butterfly, K' = max(2, the next power
 * of two >= k_r), absent lanes +0.0; k_r > 64 the 256 striding lanes, four wave butterflies, ((w0 + w1) + w2) + w3.
 * k_r == 0 gives a record of zeros.
 *
 * Output.  out holds count x 2 x (permutations + 1) records of st_dispersion_record, pair_sum holding cross_sum:
 * out[((k - begin) * 2 + dir) * (permutations + 1) + p].  A record depends on (seed, stream, p, D, set r, set c,
 * exclude_shared) alone -- not on the range, the other sets, permutations, chunk_tasks, the grid or the device; column p
 * is the same for any permutations >= p.  No float atomics.
 *
 * The caller forms, with s = |S_i and S_j| and e = exclude_shared ? s : 0:
 *     beta_mpd  = (cross_ij + cross_ji) / (2 (k_i k_j - e)),
 *     beta_mntd = (near_ij + near_ji) / (k_i + k_j - z),  z = the number of elements with no included entry,
 * either NaN where its denominator is 0.  With D[a][b] = |a - b| on 5 positions, A = {0, 1, 4} and B = {1, 2}: A -> B is
 * (cross, near) = (9, 3) and B -> A (9, 1), beta_mpd 1.5 and beta_mntd 0.8; with exclude_shared (9, 4) and (9, 2), 1.8
 * and 1.2.
 *
 * Errors are those of the dispersion pair, checked in its order (the universe size, negative permutations, chunk_tasks
 * or stream, the set table), then the range: a negative begin or count, a range outside the triangle, more than 2^31
 * pairs, more than 2^40 records (ST_ERR_ARG); the universe ids (ST_ERR_BOUNDS with *bad_id); an allocation that fails
 * is ST_ERR_NOMEM with the bytes asked for, before out is written.  Beside the dispersion call's memory the host and the
 * device hold 16 bytes per direction of the range.  chunk_tasks counts (direction, permutation) tasks.  Zero pairs, or
 * none with a member on both sides, launch nothing.
 *
 * st_beta_dispersion_matrix is the same reduction over the caller's matrix: device = -1 computes it on the host, operation
 * for operation (no GPU); device >= 0 uploads D and runs the same kernels: the same bits.  No counterpart in the reference.
 */
int st_beta_dispersion_host(st_tree *tree, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos,
                            const int64_t *sets, int64_t n_sets, int64_t begin, int64_t count, int32_t exclude_shared,
                            int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                            st_dispersion_record *out, int64_t *bad_id);

int st_beta_dispersion_matrix(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos,
                              const int64_t *sets, int64_t n_sets, int64_t begin, int64_t count, int32_t exclude_shared,
                              int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                              st_dispersion_record *out);

/*
 * How different are two sets of leaves, measured on the tree: Faith's PD of many sets over one universe and, for pairs of
 * them, the branch length of their union, from which unweighted UniFrac and PhyloSor follow.
 * SuchLinkedTrees.partner_unifrac asks it of every two leaves' partners in the other tree; SuchTree.unifrac of any sets.
 *
 * Universe.  univ (n ids, 1 <= n <= ST_UNIFRAC_MAX_UNIVERSE = 2^20) are leaves of the tree under the node `root`, in
 * depth-first order, children in increasing id order (the order of st_hommola_clades_host).  No n x n matrix is built:
 * the 16384-leaf limit of the Hommola and dispersion calls does not apply.
 *
 * Depths.  d[k] = float32 dist(root, univ[k]); h[k] = float32 dist(root, mrca(univ[k], univ[k + 1])) for k < n - 1.  Both
 * are written by the distance and MRCA kernels of the other calls, the arguments in that order: d[k] has the bits of
 * st_distances_host for the pair (root, univ[k]).  A depth that is not finite is ST_ERR_ARG.
 *
 * Fixed point.  q(v) = llrint(ldexp((double) v, shift)).  shift = -1 is automatic: 39 - ilogb(max |v|) over all of d and
 * h, and 0 when that maximum is 0, so the largest value lands in [2^39, 2^40) (for depths of 2^40 and more the shift used
 * is negative).  A caller's shift, 0 .. 256, that would put a |q| at 2^40 or more is ST_ERR_ARG.  A caller cannot pass
 * a negative shift (-1 is taken, any other negative value is ST_ERR_ARG): on a tree with a depth of 2^40 or more only
 * the automatic shift works, and range calls share one scale there only because the automatic shift of one universe
 * and root is the same in every call.  Every sum below is an
 * exact int64, |sum| < 2^61 for n <= 2^20: the results do not depend on reduction order, on which kernel form took a
 * pair, on chunk_pairs, the grid or the device.  Quantising costs at most 2^-40 of the largest depth per term, far below
 * the float32 rounding already in d.  st_unifrac_quantise is this rule on the host (out_dq[n], out_hq[n - 1], the shift
 * used; each may be NULL).
 *
 * Sets.  As for st_partner_dispersion_host: set r is the positions set_pos[sets[r] .. sets[r + 1]) of the universe,
 * strictly increasing; sets holds n_sets + 1 offsets (n_sets <= 2^30).
 *
 * Union sum of two sets A and B.  Over the distinct merged positions s_1 < ... < s_t:
 *     U(A, B) = sum over k of q(d[s_k])  -  sum over k < t of min q(h[s_k .. s_{k+1} - 1]),
 * the branch length (in units of 2^-shift) of the subtree that joins root to every member; 0 for an empty union.
 * PD(A) = U(A, A).  The caller derives the rest: shared = PD_A + PD_B - U, UniFrac = (2 U - PD_A - PD_B) / U, PhyloSor
 * = 2 shared / (PD_A + PD_B), NaN where the denominator is 0.
 *
 * Pairs.  Pair k of the sets is (j, i) with k = i (i - 1) / 2 + j, 0 <= j < i < n_sets, the order of st_triangle_host; a
 * call takes pairs [k_begin, k_begin + k_count).  out_pd holds n_sets values (every set, whatever the range), out_union
 * k_count values.  Any output may be NULL, and what is not asked for is not computed.
 *
 * st_unifrac_host checks that root and the universe ids are node ids of the tree, on the host, before anything is
 * launched (ST_ERR_BOUNDS with *bad_id).  It does not verify the rest of the precondition: a universe that is not in
 * depth-first order, an id that is not a leaf or a leaf that does not lie under root gives sums that mean nothing, with
 * no error (SuchTree.unifrac builds the universe itself and checks the members).  It then has d and h computed on the tree's device, quantises them on the host (at most 2 n values), builds the
 * range-minimum table on the device and runs the pair kernels.  out_shift is the shift used, out_d[n] and out_h[n - 1]
 * the float32 depths.  ST_ERR_ARG: n outside 1 .. ST_UNIFRAC_MAX_UNIVERSE, offsets that do not increase, a position
 * outside the universe, a set that is not strictly increasing, a range outside the triangle of n_sets (n_sets - 1) / 2
 * pairs, a negative chunk_pairs, a bad shift.  chunk_pairs: pairs per device chunk, 0 = 2^22; the result does not depend
 * on it.  Pairs of |A| + |B| <= ST_UNIFRAC_LANE_MAX positions are merged by one lane each, larger ones by one wave each;
 * the environment variable SUCHTREE_AMD_UNIFRAC_LANE_MAX (0 .. 2^22, read at every call) replaces the threshold for a
 * measurement, and no result depends on it.
 * Device memory: 8 (1 + L) n bytes of depths and table, L = floor(log2(n - 1)) + 1 levels (at most 176 MB at 2^20
 * leaves), the positions (4 bytes each) and offsets (8 bytes per set), 12 bytes per pair of a chunk for the heavy list
 * and one of the two chunks of int64 results, 8 more for the other, and 28 n bytes while the depths are computed.  An
 * allocation that fails is ST_ERR_NOMEM with the bytes asked for, before any output is written.  Zero sets launch
 * nothing (out_shift is then the caller's shift, or 0); an empty range launches no pair kernel.
 *
 * st_unifrac_depths is the same reduction over the caller's int64 arrays d_q[n] and h_q[n - 1] (a |value| of 2^40 or
 * more is ST_ERR_ARG): device = -1 is the host restatement (no GPU); device >= 0 uploads the arrays and runs the same
 * kernels: the same integers.  No counterpart in the reference.
 */
#define ST_UNIFRAC_MAX_UNIVERSE 1048576
#define ST_UNIFRAC_LANE_MAX 512

int st_unifrac_host(st_tree *tree, int64_t root, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos,
                    const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count, int32_t shift, int64_t chunk_pairs,
                    int64_t *out_pd, int64_t *out_union, int32_t *out_shift, float *out_d, float *out_h, int64_t *bad_id);

int st_unifrac_depths(int device, const int64_t *d_q, const int64_t *h_q, int32_t n, const int32_t *set_pos, int64_t n_pos,
                      const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count, int64_t chunk_pairs,
                      int64_t *out_pd, int64_t *out_union);

int st_unifrac_quantise(const float *d, const float *h, int32_t n, int32_t shift, int64_t *out_dq, int64_t *out_hq,
                        int32_t *out_shift);

/*
 * Faith's PD and the union sums of st_unifrac_host under the taxa-labels null of st_partner_dispersion_host: every set is
 * relabelled by every shuffle of the universe's labels and the sums are taken again (picante's ses.pd with null.model =
 * "taxa.labels"; the label-shuffling significance of UniFrac, Lozupone & Knight 2005).  SuchLinkedTrees.partner_unifrac_null
 * asks it of every two leaves' partners in the other tree; SuchTree.unifrac_null of any sets.
 *
 * Universe.  The universe, its order, seed, stream and sigma_p are exactly those of st_partner_dispersion_host: 3 <= n <=
 * ST_HOMMOLA_MAX_UNIVERSE leaves in depth-first order, sigma_p = st_hommola_permutation(seed, node = stream, p, side = 0,
 * n), p = 0 the identity, one sigma_p for every set of the call.
 *
 * Depths.  The depths, the fixed point, the sets and the pair order are exactly those of st_unifrac_host: d[k] the root
 * distance of univ[k], h[k] that of the MRCA of univ[k] and univ[k + 1], q(v) and shift, U(A, B) over the distinct merged
 * positions, pair k = i (i - 1) / 2 + j.
 *
 * Relabelling.  Under permutation p, set r becomes R_p(r) = { sigma_p[s] : s in set r }, taken in ascending order.
 *
 * Results.  Both arrays are int64, permutations + 1 values a row:
 *     out_pd[r * (permutations + 1) + p]                = U(R_p(r), R_p(r))   for every set r, whatever the range;
 *     out_union[(k - k_begin) * (permutations + 1) + p] = U(R_p(j), R_p(i))   for pair k = i (i - 1) / 2 + j of the range.
 * Either may be NULL, and then it is not computed.  A value depends on (the depths, shift, seed, stream, p, its one or two
 * sets) alone -- not on the other sets, the range, permutations, chunk_tasks, the kernel form, the grid or the device.
 * Column p is the same for any permutations >= p; column 0 is what st_unifrac_depths gives.  No float arithmetic on the
 * device: every sum is an exact int64.
 *
 * st_unifrac_null_host has d and h computed on the tree's device as st_unifrac_host does, quantises them on the host and
 * runs st_unifrac_null_depths' kernels on that device; out_shift is the shift used.  st_unifrac_null_depths takes the
 * caller's int64 d_q[n] and h_q[n - 1]: device = -1 is the host restatement (for each p: sigma_p, every set relabelled
 * and sorted, the merge of st_unifrac_depths; no GPU); device >= 0 runs the kernels: the same integers.
 *
 * Errors, in this order: those of st_partner_dispersion_host's first checks (a universe size outside 3 ..
 * ST_HOMMOLA_MAX_UNIVERSE, negative permutations, chunk_tasks or stream), the set table (bad offsets, a position outside
 * the universe, a set that is not strictly increasing), the range (negative, more than 2^30 sets, outside the triangle,
 * more than 2^40 values in an output array),
 * then the depths (st_unifrac_null_depths: NULL, a |value| of 2^40 or more; st_unifrac_null_host: a bad shift, NULL univ
 * or tree) -- all ST_ERR_ARG; root and the universe ids, ST_ERR_BOUNDS with *bad_id.  An allocation that fails is
 * ST_ERR_NOMEM with the bytes asked for, before any output is written.
 *
 * chunk_tasks: (set, permutation) and (pair, permutation) tasks per device chunk, and the most permutations the device
 * holds at once; 0 = the default (2^20 tasks; permutations while their sigma rows and relabelled positions, 2 bytes each,
 * stay within 64 MiB).  No result depends on it.  The relabelled positions of a block are kept on the device, set by set
 * in ascending order, for its pair tasks: 2 (permutations of the block) x n_pos bytes.  The threshold
 * between the lane and the wave form of a pair task is that of st_unifrac_host, SUCHTREE_AMD_UNIFRAC_LANE_MAX included.
 * Zero sets launch nothing (out_shift is then the caller's shift, or 0).  No counterpart in the reference.
 */
int st_unifrac_null_host(st_tree *tree, int64_t root, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos,
                         const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count, int32_t shift,
                         int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks, int64_t *out_pd,
                         int64_t *out_union, int32_t *out_shift, int64_t *bad_id);

int st_unifrac_null_depths(int device, const int64_t *d_q, const int64_t *h_q, int32_t n, const int32_t *set_pos, int64_t n_pos,
                           const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count, int64_t permutations,
                           uint64_t seed, int32_t stream, int64_t chunk_tasks, int64_t *out_pd, int64_t *out_union);

/*
 * Is one distance matrix correlated with another over the same n objects: the Mantel test, and the partial Mantel test
 * given a third matrix, under the relabelling null of st_partner_dispersion_host (compare.mantel, SuchTree.mantel,
 * SuchLinkedTrees.phylosymbiosis).  Every sum is an exact integer: "r_p >= r_0" is a comparison of integers, so the
 * p-value has no floating-point ties.
 *
 * Codes.  Both matrices enter as int32 codes.  For Pearson's form a code is q(v) = llrint(ldexp(v, shift)), the shift
 * chosen per matrix; for Spearman's form it is the doubled midrank of the m = n (n - 1) / 2 off-diagonal values minus
 * (m + 1), ranked by the caller.  Any int32 is a code.
 *
 * Orders.  x_sq is the square n x n matrix of x, C order; both triangles must be equal and the diagonal is ignored.  y
 * and z are condensed in the project's triangle order: entry k = i (i - 1) / 2 + j is the pair (i, j), 0 <= j < i < n
 * (st_triangle_host).  z = NULL is the simple test.  3 <= n <= ST_HOMMOLA_MAX_UNIVERSE.
 *
 * Permutations.  sigma_p = st_hommola_permutation(seed, node = stream, p, side = 0, n), p = 0 the identity.  x is the
 * matrix that is relabelled (vegan's mantel.partial):
 *     Sxy_p = sum over j < i of x_sq[sigma_p(i)][sigma_p(j)] * y[k(i, j)],   Sxz_p the same against z (0 without z),
 * each a 128-bit two's-complement integer in a lo / hi pair (|Sxy_p| < 2^89).  out holds permutations + 1 records, record
 * 0 the observation.  A record depends on (seed, stream, p, x_sq, y, z) alone -- not on permutations, chunk_tasks, the
 * kernel form, the grid or the device; record p is the same for any permutations >= p.
 *
 * Moments.  The sums that do not depend on p, over the pairs j < i with x = x_sq[i][j]: Sx, Sy, Sz, Sxx, Syy, Szz, Syz,
 * computed once on the host with __int128 (Sz, Szz, Syz are 0 without z).  With m pairs the caller forms
 *     r_p = (m Sxy_p - Sx Sy) / sqrt((m Sxx - Sx^2) (m Syy - Sy^2)),
 * whose order over p is that of the integers Sxy_p, and the partial coefficient from r_xy, r_xz and r_yz.
 *
 * Checked (ST_ERR_ARG), in this order: n outside 3 .. ST_HOMMOLA_MAX_UNIVERSE, negative permutations, chunk_tasks or
 * stream, more than 2^31 - 1 permutations, a NULL x_sq, y, moments or out, then an x_sq that is not symmetric, naming the
 * first cell (in row-major order) whose mirror differs; then a device below -1.  device = -1 computes every record on the
 * host (no GPU); device >= 0 uploads the matrices and runs the kernels: the same integers.  n <= 64: one wave per
 * permutation, x_sq in LDS.  Above: one workgroup per (permutation, row pair r: rows r and n - 1 - r), row sigma_p(i) of
 * x_sq staged in LDS (4 n bytes), the partial sums folded per permutation on the device; only the records cross the
 * link.  chunk_tasks: (permutation, row pair) tasks per launch, 0 = 2^20; a positive value also bounds the permutations
 * whose sigma rows the device holds at once.  Device memory: 4 n^2 bytes of x_sq, 4 m per condensed matrix, one block of
 * sigma rows (at most 64 MiB), at most 128 MiB of partial sums and 32 bytes per record; an allocation that fails is
 * ST_ERR_NOMEM with the bytes asked for, before out is written.  The environment variable SUCHTREE_AMD_MANTEL_GATHER=1
 * (read at every call) makes the row form gather from x_sq in global memory instead of staging the row, for a
 * measurement; no result depends on it.  No counterpart in the reference.
 *
 * st_mantel_quantise is the fixed point on the host: out[k] = llrint(ldexp(v[k], shift)) for n values.  shift =
 * ST_MANTEL_SHIFT_AUTO takes 30 - ilogb(max |v|), one less where the largest value would round up to 2^31, and 0 when
 * every value is 0: the largest |code| lands in [2^30, 2^31).  A caller's shift of -2000 .. 2000 that puts a |code| at
 * 2^31 or more is ST_ERR_ARG, as is a NaN or an infinity, naming its index.  out and out_shift may each be NULL.
 */
#define ST_MANTEL_SHIFT_AUTO (-2147483647 - 1)

typedef struct st_mantel_sums {
    uint64_t sxy_lo;
    int64_t sxy_hi;
    uint64_t sxz_lo;
    int64_t sxz_hi;
} st_mantel_sums;

typedef struct st_mantel_moments {
    uint64_t sx_lo;
    int64_t sx_hi;
    uint64_t sy_lo;
    int64_t sy_hi;
    uint64_t sz_lo;
    int64_t sz_hi;
    uint64_t sxx_lo;
    int64_t sxx_hi;
    uint64_t syy_lo;
    int64_t syy_hi;
    uint64_t szz_lo;
    int64_t szz_hi;
    uint64_t syz_lo;
    int64_t syz_hi;
} st_mantel_moments;

int st_mantel_codes(int device, const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, int64_t permutations,
                    uint64_t seed, int32_t stream, int64_t chunk_tasks, st_mantel_moments *moments, st_mantel_sums *out);

int st_mantel_quantise(const double *v, int64_t n, int32_t shift_or_auto, int32_t *out, int32_t *out_shift);

/*
 * Do groups of objects differ in their distances: the within-group sums of one distance matrix under the relabelling
 * null of st_mantel_codes, behind PERMANOVA and ANOSIM (compare.permanova, compare.anosim,
 * SuchLinkedTrees.partner_group_differences).  Every sum is an exact integer, so "statistic_p >= statistic_0" is a
 * comparison of integers on the caller's side.
 *
 * y holds the int32 codes of the matrix (st_mantel_quantise, or the doubled midranks minus (m + 1)), condensed in the
 * project's triangle order: entry k = i (i - 1) / 2 + j is the pair (i, j), 0 <= j < i < n.  group[i] < n_groups <=
 * ST_GROUP_MAX is the label of object i; a label that no object carries is allowed.  3 <= n <= ST_HOMMOLA_MAX_UNIVERSE.
 *
 * Permutations.  sigma_p = st_hommola_permutation(seed, node = stream, p, side = 0, n), p = 0 the identity: those of
 * st_mantel_codes.  out holds (permutations + 1) x n_groups int64 values, row 0 the observation:
 *     out[p][h] = sum over j < i with group[sigma_p(i)] == group[sigma_p(j)] == h of y[k(i, j)],
 * |sum| < 2^58.  A row depends on (seed, stream, p, y, group) alone -- not on permutations, chunk_tasks, the device, the
 * grid or the slice below; row p is the same for any permutations >= p.
 *
 * Checked (ST_ERR_ARG), in this order: n outside 3 .. ST_HOMMOLA_MAX_UNIVERSE, negative permutations, chunk_tasks or
 * stream, more than 2^31 - 1 permutations, n_groups outside 1 .. ST_GROUP_MAX, a NULL y, group or out, then the first
 * group[i] >= n_groups, named by its index; then a device below -1.  device = -1 computes every row on the host (no
 * GPU); device >= 0 uploads y and the labels and runs the kernels: the same integers.  n <= 64: one wave per permutation,
 * y in LDS.  Above: the labels are relabelled as bytes per permutation; one workgroup per (row pair r: rows r and
 * n - 1 - r, slice of permutations) stages a row of y in LDS (4 n bytes) once for the slice and compares bytes; the rows'
 * sums are folded by group per permutation on the device.  Only out crosses the link.  chunk_tasks: tasks per launch
 * (permutations, or (row pair, slice) pairs above 64 objects), 0 = 2^20; a positive value also bounds the
 * permutations whose sigma rows the device holds at once.  Device memory: 4 m bytes of y, one block of sigma rows (at
 * most 64 MiB) and half as much of labels, at most 128 MiB of partial sums and 8 n_groups bytes per row of out; an
 * allocation that fails is ST_ERR_NOMEM with the bytes asked for, before out is written.  The environment variable
 * SUCHTREE_AMD_GROUP_SLICE = 1 .. 256 (read at every call) replaces the permutations per slice, for a measurement; no
 * result depends on it.  No counterpart in the reference.
 */
#define ST_GROUP_MAX 256

int st_group_sums_codes(int device, const int32_t *y, int32_t n, const uint8_t *group, int32_t n_groups, int64_t permutations,
                        uint64_t seed, int32_t stream, int64_t chunk_tasks, int64_t *out);

/*
 * At which distances does the signal sit: the sums of one distance matrix filed under the class of each pair, under the
 * relabelling null of st_mantel_codes, behind the Mantel correlogram (compare.mantel_correlogram,
 * SuchTree.mantel_correlogram, SuchLinkedTrees.phylosymbiosis_correlogram).  One pass gives every class; every sum is
 * an exact integer, so "statistic_p >= statistic_0" is a comparison of integers on the caller's side.
 *
 * y holds the int32 codes of the matrix (st_mantel_quantise, or the doubled midranks minus (m + 1)), cls the class of
 * every pair of the other matrix, both condensed in the project's triangle order: entry k = i (i - 1) / 2 + j is the
 * pair (i, j), 0 <= j < i < n.  cls[k] < n_classes <= ST_CLASS_MAX is the class of pair k, ST_CLASS_NONE a pair that is
 * in no class; a class that no pair carries is allowed.  3 <= n <= ST_HOMMOLA_MAX_UNIVERSE.
 *
 * Permutations.  sigma_p = st_hommola_permutation(seed, node = stream, p, side = 0, n), p = 0 the identity: those of
 * st_mantel_codes, the classes relabelled as x is there.  out holds (permutations + 1) x n_classes int64 values, row 0
 * the observation:
 *     out[p][c] = sum over j < i with cls[k(sigma_p(i), sigma_p(j))] == c of y[k(i, j)]      (k(a, b) = k(b, a)),
 * |sum| < 2^58.  A row depends on (seed, stream, p, y, cls) alone -- not on permutations, chunk_tasks, the device, the
 * grid or the slice below; row p is the same for any permutations >= p.
 *
 * Checked (ST_ERR_ARG), in this order: n outside 3 .. ST_HOMMOLA_MAX_UNIVERSE, negative permutations, chunk_tasks or
 * stream, more than 2^31 - 1 permutations, n_classes outside 1 .. ST_CLASS_MAX, a NULL y, cls or out, then the first
 * cls[k] that is neither below n_classes nor ST_CLASS_NONE, named by its index; then a device below -1.  device = -1
 * computes every row on the host (no GPU); device >= 0 uploads y and the classes and runs the kernels: the same
 * integers.  n <= 64: one wave per permutation, y and the class square in LDS.  Above: the device expands the classes
 * once to the symmetric n x n byte square (rows padded to 16 bytes, the diagonal ST_CLASS_NONE); one workgroup per (row
 * pair r: rows r and n - 1 - r, slice of permutations) stages its rows of y in LDS (4 n + 16 bytes) once for the slice;
 * each of its four waves copies the square's row of the relabelled object into LDS (n bytes, padded to 16) and adds each
 * y to the 64-bit LDS accumulator of the relabelled pair's class, one set of accumulators per wave (8 KiB a workgroup):
 * 136 KiB of LDS at the limit; the row pairs' sums are folded per permutation on the device.  No global atomics.  Only out crosses the
 * link back.  chunk_tasks: tasks per launch (permutations, or (row pair, slice) pairs above 64 objects), 0 = 2^20; a
 * positive value also bounds the permutations whose sigma rows the device holds at once.  Device memory: 4 m bytes of
 * y, m bytes of classes as uploaded (128 MiB at the limit) and, above 64 objects, n rows of the square (256 MiB at the
 * limit), one block of sigma rows (at most 64 MiB), at most 256 MiB of partial sums (8 n_classes bytes per row pair and
 * permutation of a block) and 8 n_classes bytes per row of out; an allocation that fails is ST_ERR_NOMEM with the bytes
 * asked for, before out is written.  The environment variable SUCHTREE_AMD_CLASS_SLICE = 1 .. 256 (read at every call)
 * replaces the permutations per slice, and SUCHTREE_AMD_CLASS_ACC = compare runs the row form without LDS accumulators
 * that the default was measured against, each for a measurement; no result depends on either.  No counterpart in the
 * reference.
 */
#define ST_CLASS_MAX 64      /* classes per call */
#define ST_CLASS_NONE 255    /* a pair that is in no class */

int st_class_sums_codes(int device, const int32_t *y, const uint8_t *cls, int32_t n, int32_t n_classes, int64_t permutations,
                        uint64_t seed, int32_t stream, int64_t chunk_tasks, int64_t *out);

/*
 * Which links of a host-guest system carry its cophylogenetic signal: ParaFit's global statistic and ParaFitLink1 of every
 * link (Legendre, Desdevises & Bazin 2002), with their permutation counts (compare.parafit, SuchLinkedTrees.parafit).
 * Every sum is an exact integer, so every "statistic_p >= statistic_0" is a comparison of integers.
 *
 * Sides.  The links join an F (held) universe of n_f positions and an S (shuffled) universe of n_s positions.  g_f and
 * g_s are the square Gower-centred matrices G = -1/2 J D2 J of the two sides as int32 codes (st_mantel_quantise, a shift
 * per matrix), C order, both triangles equal, the diagonal meaningful.  Link l is (link_f[l], link_s[l]); the links are
 * strictly increasing in (f, s) order, so the links of one F position are one range.  3 <= n_f, n_s, n_links <=
 * ST_HOMMOLA_MAX_UNIVERSE.
 *
 * The identity.  With principal coordinates C C^T = g_s, B B^T = g_f and the link matrix A, ParaFitGlobal =
 * || C^T A B ||_F^2 = sum over links l, k of T[l][k], T[l][k] = g_f[f_l][f_k] * g_s[s_l][s_k]; removing link l lowers
 * it by ParaFitLink1(l) = 2 * (row sum of T at l) - T[l][l].  No eigendecomposition is needed.  Where a matrix has
 * negative eigenvalues their axes enter with their sign.
 *
 * Permutations.  Permutation p >= 1 redraws, for every F position i with links separately, its partners among the S
 * positions: sigma_{p,i} = st_hommola_permutation(seed, node = stream_f[i], p, side = 0, n_s), and link l = (f_l, s_l)
 * becomes (f_l, r_p(l)), r_p(l) = sigma_{p,f_l}[s_l].  The links of one F position keep distinct images; different F
 * positions draw independently (give them different stream ids).  p = 0 is the observation.  With T_p over the relabelled links:
 *     total[p]          = sum of T_p (|total| < 2^90),
 *     Link1_p(l)        = 2 * (row sum of T_p at l) - T_p[l][l]: the statistic of the relabelled link l in the relabelled system,
 *     link_obs[l]       = Link1_0(l),
 *     link_n_ge[l]      = the number of p >= 1 with Link1_p(l) >= Link1_0(l) (a tie is counted),
 *     link_all[p][l]    = Link1_p(l) for all permutations + 1 rows, where link_all is not NULL,
 * each sum a 128-bit two's-complement integer in a lo / hi pair.  A value depends on (seed, stream_f, p, the matrices, the
 * links) alone -- not on permutations, chunk_tasks, the kernel form, the grid or the device; row p is the same for any
 * permutations >= p.  ParaFitLink2 is not computed.
 *
 * Checked (ST_ERR_ARG), in this order: n_f, n_s, n_links outside 3 .. ST_HOMMOLA_MAX_UNIVERSE; negative permutations or
 * chunk_tasks; more than 2^31 - 1 permutations; a NULL g_f, g_s, link_f, link_s or stream_f; a NULL total, link_obs or
 * link_n_ge; link by link an F position, then an S position outside its universe, then a link that is not above the one
 * before (unsorted or repeated), each naming the link; the first negative stream_f[i], naming i; a g_f, then a g_s that
 * is not symmetric, naming the first cell (in row-major order) whose mirror differs; then a device below -1.
 * device = -1 computes everything on the host (no GPU); device >= 0 uploads both matrices and runs the kernels: the same
 * integers.  n_links <= 64 and n_s <= 64: one wave per permutation, g_s and the expanded held side in LDS.  Otherwise the
 * held side is expanded once to P[l][k] = g_f[f_l][f_k] (4 n_links^2 bytes) and one workgroup per (permutation, link)
 * stages row r_p(l) of g_s in LDS (4 n_s bytes).  Counts and totals are folded on the device per block of
 * permutations; total, link_obs and link_n_ge cross the link once, link_all block by block.  chunk_tasks: tasks
 * (permutations, or (permutation, link) pairs) per launch, 0 = 2^20; a positive value also bounds the permutations a
 * block holds.  Device memory: 4 n_f^2 + 4 n_s^2 + 4 n_links^2 bytes, a block of relabelled positions (at most 64 MiB)
 * and of link records (at most 128 MiB), 16 bytes per total; an allocation that fails is ST_ERR_NOMEM with the bytes
 * asked for, before any output is written.  No counterpart in the reference.
 */
typedef struct st_parafit_sum {
    uint64_t lo;
    int64_t hi;
} st_parafit_sum;

int st_parafit_codes(int device, const int32_t *g_f, int32_t n_f, const int32_t *g_s, int32_t n_s, const int32_t *link_f,
                     const int32_t *link_s, int32_t n_links, const int32_t *stream_f, int64_t permutations, uint64_t seed,
                     int64_t chunk_tasks, st_parafit_sum *total, st_parafit_sum *link_obs, int64_t *link_n_ge,
                     st_parafit_sum *link_all);

/*
 * Which clades of one tree are also in another, and how close is the best match where they are not: every induced clade
 * of tree A against every induced clade of tree B over one list of m shared leaves (SuchTree.compare_clades,
 * SuchTree.transfer_support).  The Robinson-Foulds distance, the per-clade transfer distance and the transfer bootstrap
 * expectation (Lemoine et al. 2018) follow on the caller's side.  All integers: the host restatement, the kernels and
 * any chunking give the same results.  Neither call needs a tree handle, only parent arrays.
 *
 * Order.  The m listed leaves of a tree (leaf_ids, 4 <= m <= ST_CLADE_MATCH_MAX_LEAVES = 262144) are taken depth-first,
 * children in increasing id order (the order of st_unifrac_host's universe): position k is the k-th listed leaf met,
 * and out_order[k] its index in leaf_ids.
 *
 * Induced clades.  c(v) = listed leaves under internal node v.  v is kept when c(v) >= 2 and no child of v has the same
 * count: v is then the MRCA of its set, and unlisted leaves collapse away.  A kept node is the position range [lo, hi)
 * of size s = hi - lo.  Kept nodes are listed breadth-first from the root, children in increasing id order (the order of
 * SuchTree.get_internal_nodes()).  A binary tree has m - 1 of them.  Eligible, for rows and candidates alike:
 *     rooted:   kept nodes with 2 <= s <= m - 1;
 *     unrooted: kept nodes with 2 <= s <= m - 2, and the node whose range is [k, m) is left out when [0, k) is also
 *               eligible (the root's two children are one bipartition).
 *
 * st_clade_ranges (host only) writes the order and the eligible clades of one tree: out_node / out_lo / out_hi need room
 * for m - 1 entries (there are never more), *out_n is their number.  The parent array is that of st_clade_plan (int32,
 * -1 at the one root; ST_ERR_TREE when it is not one rooted tree).  ST_ERR_BOUNDS with *bad_id for an id outside
 * [0, n_nodes); ST_ERR_ARG with *bad_id for an id that is not a leaf or is listed twice, and for m out of range.
 *
 * Distance.  For row a of A and candidate b of B, with pos_b[k] = B's position of the leaf at A's position k:
 *     i = |a n b| = #{k in [a_lo, a_hi) : b_lo <= pos_b[k] < b_hi},  d = s_a + s_b - 2 i,
 *     delta(a, b) = d (rooted) or min(d, m - d) (unrooted).
 * The row's result is the candidate of least delta, a tie going to the lower index in B's list: the minimum of the key
 * delta << 32 | index, so no reduction order matters.  out_distance / out_match / out_intersection (n_a each) are delta,
 * the index and i of that candidate; -1, -1 and 0 when n_b = 0.  The caller derives, with p = s_a (rooted) or
 * min(s_a, m - s_a) (unrooted): transfer = min(delta, p - 1) (p - 1 without a candidate), support = 1 - transfer / (p - 1),
 * exact = rows of delta 0, RF = n_a + n_b - 2 exact.
 *
 * st_clade_match: device = -1 is the host restatement (no GPU, one thread, a prefix count per row); device >= 0 runs
 * k_clade_match, one row per workgroup: a bitmap of the row's B positions and one running count per 64-bit word in
 * LDS (12 bytes per 64 leaves: 48 KiB at the cap), two rank lookups per candidate.  B's candidates are sorted by size on
 * the host (stable); since delta >= |s_a - s_b| (and >= |m - s_a - s_b| by the complement when unrooted) a row first
 * scans only the size windows that can beat p - 1 and falls back to all candidates when nothing there does, so the true
 * minimum is reported either way.  The environment variable SUCHTREE_AMD_CLADE_MATCH_WINDOW (0 or 1, read at every
 * call) turns the windows off or on for a measurement; no result depends on it.  chunk_rows: rows per launch and
 * read-back, 0 = 65536; no result depends on it.
 * Checked (ST_ERR_ARG): m in range, counts and chunk_rows not negative, NULL arrays, pos_b a permutation of 0 .. m - 1,
 * every range 0 <= lo < hi <= m.  Not verified: that the ranges of either list form a laminar family, are distinct, or
 * come from st_clade_ranges -- any list of ranges is matched as it stands.
 * Device memory: 4 m bytes of positions, 12 bytes per candidate, 24 per row, and two chunks of 12 bytes per row of
 * results.  An allocation that fails is ST_ERR_NOMEM with the bytes asked for, before any output is written.  n_a = 0
 * launches nothing.  No counterpart in the reference, which offers bipartitions() as Python sets (MuchTree.pyx:1151-1200).
 */
#define ST_CLADE_MATCH_MAX_LEAVES 262144

int st_clade_ranges(const int32_t *parent, int64_t n_nodes, const int64_t *leaf_ids, int32_t m, int32_t rooted,
                    int32_t *out_order, int32_t *out_node, int32_t *out_lo, int32_t *out_hi, int32_t *out_n, int64_t *bad_id);

int st_clade_match(int device, int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a,
                   const int32_t *b_lo, const int32_t *b_hi, int32_t n_b, int32_t unrooted, int64_t chunk_rows,
                   int32_t *out_distance, int32_t *out_match, int32_t *out_intersection);

/*
 * Exact agglomerative clustering of a distance matrix of int32 codes: UPGMA ("average"), single and complete linkage.
 * Every quantity is an integer, so the dendrogram is a function of the codes alone: a tie is a real tie, broken by the
 * rule below, on the host and on the device alike.
 *
 * Input: n objects, 2 <= n <= ST_LINKAGE_MAX_OBJECTS; codes[i (i - 1) / 2 + j] >= 0 is the code of pair (i, j), j < i;
 * weights is NULL or n values >= 1 with a total of at most ST_LINKAGE_MAX_WEIGHT -- object i then stands for weights[i]
 * coincident objects.  The bound keeps every pair sum below 2^62 and every cross product below 2^92.
 *
 * Clusters live in slots.  Slot i starts as object i: size s_i = weights[i] (1 without weights), cluster id i.  S(i, j)
 * starts as codes(i, j) s_i s_j for ST_LINKAGE_AVERAGE and as codes(i, j) for ST_LINKAGE_SINGLE and ST_LINKAGE_COMPLETE.
 * The value of an active pair is the fraction S(a, b) / (s_a s_b) (average) or S(a, b) / 1 (single, complete); two
 * values compare by cross-multiplication in 128 bits.  Step t = 0 .. n - 2:
 *   1. of the active pairs a < b take the one of least value; on a tie the least a, then the least b;
 *   2. out_rows[t] = {num, den, left, right, size}: num / den the value as above (not reduced), left < right the two
 *      cluster ids, size = s_a + s_b;
 *   3. slot a holds the merged cluster, id n + t, size s_a + s_b; slot b dies; every other active slot k gets
 *      S(k, a) = S(k, a) + S(k, b) (average), min (single) or max (complete) of the two.
 * The three methods are reducible, so the values never decrease along t.  left, right and size are those of
 * scipy.cluster.hierarchy.linkage's Z where scipy meets no tie.
 *
 * Checked (ST_ERR_ARG), in this order: n out of range, an unknown method, codes or out_rows NULL, the first negative code
 * (naming its index), the first weight below 1 (naming its index), a total weight above ST_LINKAGE_MAX_WEIGHT.
 * device = -1 is the host restatement (no GPU: a nearest-later-partner cache per slot, repaired after every merge, not
 * the scan of all pairs); device >= 0 runs the kernels there -- the same integers.  Device memory is the square int64
 * S, 8 n (n + 63) bytes at most (2 GiB at the limit), the codes and 16 n bytes of cache; an allocation that fails is ST_ERR_NOMEM with
 * the bytes asked for, before out_rows is written.  The chain of merges is serial: on the device it is one workgroup
 * that synchronises with workgroup barriers only.  The environment variable SUCHTREE_AMD_LINKAGE_CACHE = lds / global
 * (read at every call) says where that workgroup keeps the cache, for a test or a measurement: no result depends on it,
 * and above the n that fits LDS it is global whatever is asked.  No counterpart in the reference.
 */
#define ST_LINKAGE_MAX_OBJECTS 16384
#define ST_LINKAGE_MAX_WEIGHT  65536
#define ST_LINKAGE_AVERAGE  0
#define ST_LINKAGE_SINGLE   1
#define ST_LINKAGE_COMPLETE 2

typedef struct st_linkage_row {
    int64_t num, den;       /* the value of the merge: num / den, den = s_a s_b (average) or 1 */
    int32_t left, right;    /* the two cluster ids, left < right */
    int64_t size;           /* s_a + s_b */
} st_linkage_row;

int st_linkage_codes(int device, const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, st_linkage_row *out_rows);

/*
 * Which clades do the trees of a set share, pair by pair: the exact count behind the Robinson-Foulds distance between
 * every two trees of a set (bootstrap replicates, a posterior sample, dendrograms under several measures), behind the
 * number of trees that hold each clade, and behind the Robinson-Foulds column of a relabelling test (compare.tree_set,
 * compare.rf_relabelled).  Only identical clades are counted, not the closest one (that is st_clade_match), so the method
 * is Day's: near-linear per pair of trees, all integers.  The call needs no tree handle, only positions and ranges.
 *
 * Input.  One list of m common leaves, 4 <= m <= ST_RF_MAX_LEAVES = 16384 (a position fits 16 bits; above it
 * st_clade_match per pair is the route), and n_trees trees.  For tree t, where[t * m + k] is the depth-first position in
 * t of common leaf k (the inverse of st_clade_ranges' out_order), and its eligible clades are the ranges lo / hi at
 * [clade_offsets[t], clade_offsets[t + 1]) of one concatenated list: what st_clade_ranges writes for the same `unrooted`
 * flag, after any filter of the caller's.  align is NULL or n_align rows of m int32, each a permutation of 0 .. m - 1.
 * Tasks come in one of two forms: the arrays task_i, task_j (and task_p, which may be NULL: the identity everywhere) of
 * length n_tasks, task_p[t] = -1 being the identity and begin being 0; or, with all three NULL, the n_tasks pairs
 * [begin, begin + n_tasks) of the triangle in the order k = i (i - 1) / 2 + j, j < i, under the identity.
 *
 * A task (i, j, p), with a = align[p] or the identity: common leaf k of tree i meets common leaf a[k] of tree j.  For
 * clade b of j, Q_b = { where_i[k] : lo_b <= where_j[a[k]] < hi_b }.  b is shared when some clade c of i has
 * [lo_c, hi_c) = Q_b (rooted), or = Q_b or its complement in [0, m) (unrooted).  out_shared[task] is the number of shared
 * b.  With lists from st_clade_ranges this is the number of rows of delta 0 of st_clade_match over the same two sides and
 * alignment, in either direction, and RF = n_i + n_j - 2 shared.  i = j with the identity gives n_i.
 * out_count (int64, one per clade of the concatenated list; NULL skips it) is zeroed, then every shared b of every task
 * adds 1 to its own entry and 1 to the entry of the matching c (the first in i's list, should a caller's list repeat a
 * set).  The additions are integers: their order does not matter.  Over the whole triangle, entry c of tree t ends as
 * the number of other trees that hold the clade.
 *
 * Method.  q[where_j[a[k]]] = where_i[k] is one scatter of m entries; Q_b = q[lo_b .. hi_b) is a range if and only if
 * max - min + 1 = size, and then the range [min, max + 1) is looked up in tree i's list, sorted once per call.  Unrooted,
 * every key is the side without i's position 0: a range of i's list that starts at 0 is stored as [hi, m), and a clade of
 * j that holds the leaf at i's position 0 is tested through its complement, the two ranges [0, lo_b) and [hi_b, m).
 * device = -1 is the host restatement (no GPU, one thread, the same tables); device >= 0 runs k_rf_tasks, one task per
 * workgroup: q as 16-bit entries in LDS, min and max per block of 64 positions, a sparse table over the at most 256 blocks
 * (9 levels), so that the extrema of a range are two partial blocks and two table entries; a binary search per clade in
 * tree i's keys (global memory); 2 m + 16 bytes of LDS and at most 9 KiB of table, 42,000 bytes at the cap.
 * chunk_tasks: tasks per launch and read-back, 0 = 65536, at most 2^24 (more is cut to that); no result depends on it.
 *
 * Checked, before anything is launched or written (ST_ERR_ARG, naming the cell): m in range; no negative count, begin or
 * chunk_tasks; no NULL where an array is needed; clade_offsets from 0, non-decreasing, below 2^31; every row of where a
 * permutation of 0 .. m - 1; every range 0 <= lo < hi <= m; every row of align a permutation; task_i and task_j given
 * together and begin = 0 with them; every tree index and every alignment index of a task in range (ST_ERR_BOUNDS, naming
 * the task); the triangle range inside n_trees (n_trees - 1) / 2; out_shared.  Not verified: that a tree's ranges form a
 * laminar family, are distinct, or come from st_clade_ranges -- any list of ranges is processed as it stands.
 * Device memory: 2 m bytes per tree and per alignment row, 12 bytes per clade, 4 (n_trees + 1) bytes of offsets, 12 bytes
 * per explicit task, 8 bytes per clade with out_count, and two chunks of 4 bytes per task of results.  An allocation that
 * fails is ST_ERR_NOMEM with the bytes asked for, before any output is written.  n_tasks = 0 launches nothing.  A tree
 * without clades (a star) shares 0.  No counterpart in the reference, which offers bipartitions() as Python sets.
 */
#define ST_RF_MAX_LEAVES 16384

int st_rf_tasks(int device, int32_t m, int32_t n_trees, const int32_t *where, const int64_t *clade_offsets, const int32_t *lo,
                const int32_t *hi, int32_t unrooted, const int32_t *align, int32_t n_align, const int32_t *task_i, const int32_t *task_j,
                const int32_t *task_p, int64_t n_tasks, int64_t begin, int64_t chunk_tasks, int32_t *out_shared, int64_t *out_count);

/*
 * Exact Spearman rank correlation of the same pairs.  rank_x is the midrank of x_k among the call's n float32 distances
 * (scipy.stats.rankdata(x, "average"): equal values tie, -0.0 ties with +0.0), a_k = 2 rank_x(x_k) - (n + 1)
 * = 2 (#values < x_k) + (#values == x_k) - n, an integer, and b_k likewise for y.  Then
 *   Sxy = sum a_k b_k,   Sxx = sum a_k^2 = (n^3 - n - sum over x's tie groups of (t^3 - t)) / 3,   Syy likewise,
 * and Spearman's rs = Sxy / (sqrt(Sxx) sqrt(Syy)): NaN when Sxx or Syy is 0, when n < 2 or when n_nan > 0 (scipy's
 * "propagate").  The three sums are 128-bit two's-complement integers: they do not depend on reduction order, grid,
 * chunk size or device, so two calls, or a call and st_spearman_host on the same values, agree exactly.
 *
 * No pair is kept.  Three passes recompute the distances chunk by chunk: the first is st_compare_*_host's own (out
 * receives the same st_pair_moments, bit for bit, as that call without a histogram) and also marks which of the 4096
 * top-12-bit buckets of the order-preserving key each tree's values fall in; the second counts every value in one
 * uint32 counter per (occupied bucket, low 20 bits) and a scan in key order turns the counts into a_k in place; the
 * third looks a_k and b_k up and sums their products.  Device memory: the chunk plus 4 MiB per occupied bucket and tree
 * (ml.tree vs nj.tree, all pairs: 0.6 GB; at worst 2 x 4096 buckets, 32 GiB) -- it does not grow with the pair count.
 * n is limited to 2^31 - 1 (|a| within int32, a b within int64): more is ST_ERR_ARG and launches nothing.
 * chunk_pairs: pairs per device chunk of the second and third pass, 0 = the path's default, else a positive multiple
 * of ST_CLADE_TILE (ST_ERR_ARG otherwise); the result does not depend on it.  Pairs, orientation, id checks and error
 * codes are those of st_compare_triangle_host / st_compare_pairs_host.  No counterpart in the reference, whose docs
 * rank a sample of the pairs on the host (scipy.stats.spearmanr).
 */
typedef struct st_rank_sums {
    int64_t  n, n_nan;                 /* pairs ranked; pairs with a NaN on either side (then everything below is 0) */
    int64_t  distinct_x, distinct_y;   /* distinct values after -0 -> +0 */
    uint64_t sxy_lo; int64_t sxy_hi;   /* 128-bit two's complement */
    uint64_t sxx_lo, sxx_hi, syy_lo, syy_hi;
} st_rank_sums;
int st_compare_triangle_ranks_host(st_tree *tree_x, st_tree *tree_y, const int64_t *ids_x, const int64_t *ids_y, int64_t m,
                                   int64_t k_begin, int64_t k_count, int64_t chunk_pairs,
                                   st_pair_moments *out, st_rank_sums *out_ranks, int64_t *bad_id);
int st_compare_pairs_ranks_host(st_tree *tree_x, st_tree *tree_y, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n,
                                int64_t chunk_pairs, st_pair_moments *out, st_rank_sums *out_ranks, int64_t *bad_id);
/* Host only, no GPU: the same keys, midranks and tie arithmetic over two plain arrays of n values. */
int st_spearman_host(const float *x, const float *y, int64_t n, st_rank_sums *out);

/*
 * Exact Kendall's tau-b of the same pairs (scipy.stats.kendalltau(x, y), variant "b", nan_policy "propagate"), from
 * integer counts over the call's n pairs of float32 distances.  With n0 = n (n - 1) / 2:
 *   ties_x     = sum over the tie groups of x of t (t - 1) / 2 (equal values tie, -0.0 ties with +0.0; infinities are
 *                ordinary values), ties_y likewise, ties_xy over the groups equal in both x and y,
 *   discordant = the number of {i, j} with (x_i - x_j)(y_i - y_j) < 0,
 *   concordant = n0 - ties_x - ties_y + ties_xy - discordant,
 *   tau        = (concordant - discordant) / sqrt((n0 - ties_x)(n0 - ties_y)): NaN when a factor is 0, when n < 2 or when
 *                n_nan > 0 -- then every count is 0, as in st_rank_sums.
 * Every count is an integer below 2^61 (n <= 2^31 - 1: more is ST_ERR_ARG and launches nothing): none depends on
 * reduction order, grid, chunk size or device, so two calls, or a call and st_kendall_host on the same values, agree
 * exactly.
 *
 * The pairs are kept and sorted on the device: one pass of the distance kernels writes each pair's 64-bit key (the
 * order-preserving key of x above that of y) -- out receives the same st_pair_moments, bit for bit, as
 * st_compare_*_host without a histogram -- then a merge sort by (x, y) (tiles of ST_KENDALL_TILE keys in LDS, then
 * merge-path levels), the x and joint tie sums from runs of the sorted keys, a second merge sort of the low words that
 * counts inversions (= discordant), and ties_y from its result.  Device memory: 16 bytes per pair beside the chunk (ml.tree
 * vs nj.tree, all 1,475,684,301 pairs: 24 GB; at the limit 34 GB); an allocation that fails is ST_ERR_NOMEM and says how
 * many bytes were asked for.  chunk_pairs, pairs, orientation, id checks and error codes: as for st_compare_*_ranks_host.
 * No counterpart in the reference, whose docs call scipy.stats.kendalltau on a host-side sample of the pairs.
 */
#define ST_KENDALL_TILE 2048   /* keys a workgroup sorts in LDS and a merge level's workgroup writes */
typedef struct st_kendall_counts {
    int64_t  n, n_nan;                 /* pairs counted; pairs with a NaN on either side (then everything below is 0) */
    uint64_t discordant, ties_x, ties_y, ties_xy;
} st_kendall_counts;
int st_compare_triangle_kendall_host(st_tree *tree_x, st_tree *tree_y, const int64_t *ids_x, const int64_t *ids_y, int64_t m,
                                     int64_t k_begin, int64_t k_count, int64_t chunk_pairs,
                                     st_pair_moments *out, st_kendall_counts *out_counts, int64_t *bad_id);
int st_compare_pairs_kendall_host(st_tree *tree_x, st_tree *tree_y, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n,
                                  int64_t chunk_pairs, st_pair_moments *out, st_kendall_counts *out_counts, int64_t *bad_id);
/* The counts of two plain float32 arrays of n values: both are uploaded to `device` and go through the same kernels. */
int st_kendall_arrays_host(int device, const float *x, const float *y, int64_t n, st_kendall_counts *out);
/* Host only, no GPU: the same keys, tie rule and counts. */
int st_kendall_host(const float *x, const float *y, int64_t n, st_kendall_counts *out);

/*
 * Quartet topologies: for each row (a,b,c,d) of the int64 (n,4) view the row re-ordered so
 * that columns (0,1) and (2,3) are the sister pairs.  Replaces
 * SuchTree._quartet_topologies (SuchTree/MuchTree.pyx:1331-1376) as called by
 * quartet_topologies_bulk (:1271-1329).  out_topologies is C-order int64 (n,4).
 */
int st_quartets_host(st_tree *tree, const int64_t *quartets, int64_t n,
                     int64_t stride0, int64_t stride1,
                     int64_t *out_topologies, int64_t *bad_id);

/*
 * Compare two trees by quartet topology, counted on the GPU.  The quartets are generated on the device (or uploaded),
 * classified in both trees by the MRCA kernels behind st_quartets_host, and counted: only the table leaves the device.
 * Replaces, for the question "how many quartets do two trees resolve alike", two quartet_topologies_bulk calls
 * (SuchTree/MuchTree.pyx:1271-1329) and a host-side comparison of their (n,4) results.  No counterpart in the reference.
 *
 * Class of a quartet (a,b,c,d) in one tree.  Take the six MRCA ids in the reference's order ab ac ad bc bd cd
 * (MuchTree.pyx:1357-1362) and let `pick` be the first index whose id occurs exactly once among the six (the rule of
 * _quartet_topologies, :1364-1372).  Class 0 is ab|cd (pick 0 or 5), class 1 ac|bd (pick 1 or 4), class 2 ad|bc (pick 2
 * or 3); class 3 is "none unique", where the reference leaves j = 5 and reports ab|cd -- counted apart here.  Four
 * distinct leaves never give class 3; repeated ids and internal nodes may.
 *
 * Result.  cell[i][j] counts the quartets of class i in tree_x and class j in tree_y; n is the sum of the cells.  The
 * counts are integers accumulated with integer atomics: they do not depend on grid, chunking, device or order, and two
 * calls over disjoint index ranges add cell by cell to the call over their union.
 *
 * ST_QUARTET_ALL: all quartets of m leaves.  Quartet k, 0 <= k < C(m,4), is the k-th 4-subset of positions
 * p0 < p1 < p2 < p3 in colexicographic order: p3 is the largest p with C(p,4) <= k, then k -= C(p3,4); p2 the largest p
 * with C(p,3) <= k, and so on down to p0.  The quartet is (ids[p0], ids[p1], ids[p2], ids[p3]).  4 <= m <= 65536, so
 * that C(m,4) < 2^60; m < 4 is valid only with a count of 0.
 *
 * ST_QUARTET_SAMPLE: sampled quartets.  Quartet k depends on (seed, k, m) alone, so the first k quartets are the same
 * for any sample size.  For j = 0..3, u_j = mix(seed + (4k + j + 1) * 0x9E3779B97F4A7C15 mod 2^64), mix the splitmix64
 * finalizer (z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31), and r_j = the high
 * 64 bits of u_j * (m - j).  p_j starts as r_j; going through the positions already chosen in increasing order,
 * p_j++ whenever p_j >= q.  The quartet is (ids[p_0], ..., ids[p_3]) in draw order: an ordered 4-tuple of distinct
 * positions, uniform up to m * 2^-64.  4 <= m < 2^31 and k_begin + k_count <= 2^62; m < 4 only with a count of 0.
 */
#define ST_QUARTET_ALL     0
#define ST_QUARTET_SAMPLE  1
typedef struct st_quartet_table {
    int64_t n;             /* quartets counted: the sum of the cells */
    int64_t cell[4][4];    /* [class in tree_x][class in tree_y] */
} st_quartet_table;

/* The (k_count,4) int32 positions of quartets [k_begin, k_begin + k_count) of `mode`.  device = -1 computes them on the
 * host (no GPU, no tree); device >= 0 runs the generator kernel of the compare path and copies its output back: the same
 * values.  It states which quartets a sample held.  A bad mode, m or range is ST_ERR_ARG, as is a NULL out_pos with
 * k_count > 0. */
int st_quartet_positions(int device, int mode, uint64_t seed, int64_t m, int64_t k_begin, int64_t k_count, int32_t *out_pos);

/* Generated quartets [k_begin, k_begin + k_count) over two aligned id lists: quartet positions (p0..p3) are evaluated as
 * (ids_x[p0..p3]) in tree_x and (ids_y[p0..p3]) in tree_y.  The ids need not be leaves.  Conventions as for
 * st_compare_triangle_host: both trees on one device (tree_x == tree_y allowed); every id is checked on the host before
 * anything is launched (ST_ERR_BOUNDS with *bad_id, tree_x's ids first); an empty range gives a zero table and launches
 * nothing.  chunk_quartets: quartets per device chunk, 0 = the default, else a positive value below 2^31 / 6; the result
 * does not depend on it.  A bad mode, m, range or chunk is ST_ERR_ARG.  Device memory is bounded by the chunk -- two
 * (c,4) int64 id arrays, two 6c int32 MRCA arrays, the table -- plus the two id lists. */
int st_compare_quartets_leaves_host(st_tree *tree_x, st_tree *tree_y, const int64_t *ids_x, const int64_t *ids_y, int64_t m,
                                    int mode, uint64_t seed, int64_t k_begin, int64_t k_count, int64_t chunk_quartets,
                                    st_quartet_table *out, int64_t *bad_id);
/* Explicit quartets: row i of the C-order int64 (n,4) array quartets_x in tree_x against row i of quartets_y in tree_y,
 * uploaded chunk by chunk.  Otherwise as above. */
int st_compare_quartets_host(st_tree *tree_x, st_tree *tree_y, const int64_t *quartets_x, const int64_t *quartets_y, int64_t n,
                             int64_t chunk_quartets, st_quartet_table *out, int64_t *bad_id);

/*
 * Dense graph matrices of SuchLinkedTrees: adjacency A (A[u][v] = A[v][u] = w per edge) and
 * Laplacian L = diag(column sums of A) - A, both n x n float64, C order; either output may
 * be NULL.  Replaces the numpy assembly at the end of SuchLinkedTrees.adjacency / .laplacian
 * (SuchTree/MuchTree.pyx:3110-3145); the edge list (tree edges normalised by the largest
 * edge, link edges at the mean weight, :3113-3129) is prepared by the caller.  No tree
 * handle involved.
 */
int st_graph_matrices_host(int device, int64_t n, int64_t n_edges, const int32_t *u,
                           const int32_t *v, const double *w,
                           double *out_adjacency, double *out_laplacian);

/* Select the kernel family for subsequent calls (tests / benchmarking).
 * ST_ERR_ARG if the tree was built without that family's tables. */
int st_tree_set_strategy(st_tree *tree, int strategy);

/* Tuning knobs (benchmarking / tests).
 * "tile_sort": 1 = on deep canopies whose records hold at most seven chain slots (16- to 64-byte records: small deep trees, a
 * few thousand leaves) every workgroup sorts its tile of pairs by expected climb length so that a wave's lanes finish together
 * (the default where it measured fastest when the tree was created, see "prefer_walk_sorted" below); 0 = pairs in input order.
 * On longer records the option selects nothing since version 6: the tile-sorted canopy kernel's 15- / 31-slot and pointer forms
 * won no cell of profiles/kernel_win_matrix_r06.json against the scalar ladder kernel ("ladder_scalar") and were removed.
 * "tree_rmq": 1 (default) = the walk family takes the meeting node from the whole-tree sparse table
 * where the tree has one (in-order ids; up to 64 MB, more -- within SUCHTREE_AMD_WALK_TABLE_MB -- when
 * the canopy family is not available); 0 = it searches it by climbing both lineages.
 * "mrca_ranks": 1 (default) = MRCA-only requests on trees with in-order ids are answered from a
 * per-node rank table and a sparse table over the canopy (no LDS, no understory records);
 * 0 = they go through the distance kernels.
 * "lineage_sums": 1 (default) = the first node's whole side of a pair comes from a table of per-node
 * lineage sums (one 4-byte read) wherever the tree has that table: in the tile-sorted canopy kernel
 * (deep canopies with in-order ids, table below 1 GiB) and in the walk family (the same trees, and
 * trees only the walk family serves); 0 = that side is climbed as well (this also switches off
 * everything below that builds on the table).
 * "lineage_lens": 1 (default) = the walk family adds the second node's side from the lineage-length
 * table, consecutive floats, instead of climbing the stride-3 image; 0 = it climbs.
 * "walk_crown": 1 (default) = the walk family reads the long upper part of that stream from the
 * block of the node's portal (shared by all nodes below it: a cache-resident hot set) and takes
 * meeting nodes of different portals from the crown's own sparse table; 0 = own block, whole-tree table.
 * "walk_ladder": 1 (default) = where the crown is small enough (<= 8192 nodes) the tile-sorted walk kernel keeps
 * its ladder form in LDS and climbs the upper part of the second node's side there (three edges per 16-byte LDS
 * read) instead of streaming it; 0 = it streams it from the portal's block.
 * "walk_sort": 1 (default) = batches of >= 262144 pairs on trees with the sparse table and both lineage
 * tables run the tile-sorted walk kernel (a wave's 64 pairs have streams of similar length); 0 = k_walk.
 * "prefer_walk_sorted": 1 = distance batches of >= 524288 pairs on a canopy-strategy tree that also has the walk
 * family's tables (deep trees) go to the tile-sorted walk kernel; 0 = they stay with the canopy kernels.  Like
 * "tile_sort" its default is set when the tree is created, on deep trees by timing the candidate
 * kernels on a sample of random leaf pairs (st_tree_info.tuned; SUCHTREE_AMD_AUTOTUNE=0: by a fixed rule).
 * "ladder_scalar": 1 = distance batches of at least "ladder_min_pairs" pairs (0 = 131072) on records of 128 bytes and
 * more are served by the scalar kernel over the ladder form of the canopy (records read once, no sort: large batches);
 * both defaults are set with the three above when a deep tree is created (timed at two or three batch sizes, on
 * uniform random leaf pairs: a caller whose batches are all close relatives -- every pair within a few leaves, short
 * paths -- does better with "ladder_scalar" 0 and "prefer_walk_sorted" 1: the walk family's cost follows the path
 * length; nj.tree, leaves within 8 of each other: 1.4e10 -> 1.9e10 pairs/s, ml.tree 1.7e10 -> 2.0e10).
 * "ladder_sums": 1 = that kernel reads the first node's whole side of a pair from the lineage sums (one 4-byte read in place of
 * its understory entry and its climb in LDS; the meeting node from the 64-bit sparse table by the two portal ranks, the second
 * node's record by the 16-byte chunks that hold chain slots in use) and climbs the second node's canopy edges only; 0 = both
 * sides are climbed.  Needs the lineage sums ("lineage_sums" 1, table built); the default is set by timing when a deep tree is
 * created, possibly for batches up to a size only (nj.tree: 1, +17 %; ml.tree: 1 for batches below 2^20 pairs, where it leads
 * by 8-13 %, 0 above -- there the extra fabric read costs more than its second workgroup's climbs save); setting the option by
 * hand applies it to every batch size.
 * "ladder_dynamic": 1 (default) = on records of 512 bytes and more, batches of 2^22 pairs and more (2^21 on 1 KB
 * records) of that kernel draw their work from per-XCD counters instead of a static deal; 0 = never.
 * "walk_sort_min": smallest batch (pairs) that kernel takes; 0 (default) = 262144.
 * "sort_tile": tile of both tile-sorted kernels in units of 1024 pairs: 1, 2 or 4 (taken when it fits LDS and the
 * kernel's form has that tile), 0 (default) = the largest tile LDS admits, cut finer for batches that would
 * otherwise leave CUs without a tile.
 * "rec_a4": 1 (default) = on trees whose leaves sit in portal-uniform aligned blocks of leaf slots (balanced
 * and near-balanced trees) the predicated canopy kernel gathers 4 bytes for the first node of a pair
 * (its understory sum; the portal comes from a block table in LDS) instead of the 8-byte entry; 0 = 8 bytes.
 * "cherries": 1 (default) = on such trees the second node of a pair, when it is a leaf whose block of leaf slots consists
 * of sibling pairs, is read from the pair's cherry record (one record of rec_b's size per two leaves: half the table);
 * 0 = from rec_b.
 * "heap_lines": perfect trees with in-order ids and 6 to 20 levels of edges also get heap lines -- one 128-byte line per 16
 * leaves that holds the 31 edges of their subtree and the one above it, and the levels above as a heap kept in LDS: every
 * edge once, 8 bytes per leaf.  Explicit pair batches with distances then read both nodes of a pair from that table, with
 * ids, MRCAs and meeting depths by arithmetic (the same bits).  1 (default) = on trees of 2^17 leaves and more (at 2^16 the
 * tables above are still ahead); 2 = wherever the tables exist; 0 = never.  st_tree_info.heap_lines
 * follows.  Under a table budget these tables are the first to go.
 * "heap_codes": where every edge length of such a tree is a six-decimal number below 1.048576 (a Newick file with six decimals)
 * the six lowest levels are also kept as 20-bit integer codes, 24 leaves per 128-byte line -- two thirds of the heap lines'
 * footprint; every edge is verified to decode to its own bits, else the table is not built.  The batches that take the heap-line
 * form then read it instead (the same bits).  1 (default) = batches of 2^24 pairs and more on trees of 2^19 leaves and more; 2 = wherever the table exists
 * and "heap_lines" admits the heap-line form; 0 = never.  "heap_lines" 0 turns both forms off.  st_tree_info.heap_codes
 * follows; heap_lines, a_side_bytes, b_table_bytes_per_leaf and stream_hint report what they report without it.  Under a
 * table budget this table goes before the heap lines.
 * "stream_hint": the pair array and the result arrays of a launch are read once and written once; with the hint the kernel
 * reads and writes them non-temporally, so that they do not push the tables it gathers from out of L2 (the same bytes either
 * way).  1 (default) = explicit pair batches from and to device buffers (st_distances_device, _f32, _wire) that the
 * heap-line kernel takes: pair loads and result stores; 2 = also the pair loads of the predicated kernel on general tables, for
 * such batches and for the host entry points' int32 pairs (the other kernels have no hinted form); 0 = never.  Paths whose next kernel reads the results
 * back (the st_compare_* family) never use it.  st_tree_info.stream_hint follows.
 * "wire48": 1 (default) = on trees of fewer than 2^24 nodes the host entry points ship ids over the link as 24 bits
 * each (6 bytes per pair instead of 8; the packing step then checks the range and keeps the id to report); 0 = int32.
 * "wire24": 1 (default) = on such trees MRCA ids come back over the link as 24 bits each (7 bytes per pair with the
 * float32 distance instead of 8; assembled by the kernels, widened by the host's unpack pass); 0 = int32.
 * "reserve_cus": CUs the launches leave to others (default 0): the kernels are persistent workgroups sized to the
 * device; a rank that receives result slices while it computes (the root of the multi-GPU gather) can leave RCCL's
 * kernels a few CUs of their own.
 * "small_batch_path": 1 (default) = host batches of <= 8192 pairs go through a pinned,
 * device-mapped mailbox (one launch; completion is polled in host memory), 0 = through the
 * staged pipe.
 * "batch_probe": 1 (default) = on deep trees whose handle sends large distance batches to the scalar ladder kernel and
 * whose tile-sorted walk kernel is ready as well, every device-resident batch of >= 2^22 explicit pairs is sampled on the device
 * (1024 pairs, one from every 1024th of the batch at a hashed offset: do both nodes share their portal?) and goes to the walk
 * kernel when a quarter of the sample does -- batches of close relatives -- else to the ladder kernel.  Both kernels are enqueued
 * and every workgroup of either takes the sample itself; the kernel it does not choose returns at once: no probe launch, no host
 * round trip, 8-10 us per batch (version 5's separate probe kernel, from 524288 pairs: 20 us).  0 = always the handle's choice.
 * "measure" (default 0; MEASUREMENT ONLY): bits 1 = one line per host-path call on stderr with the host thread's time by
 * phase, 2 = the host path skips its pack / unpack passes, 4 = it launches nothing.  A call made with bit 2 or 4 set
 * returns ST_ERR_MEASURE_ONLY, never ST_OK: its result arrays are not valid. */
int st_tree_set_option(st_tree *tree, const char *name, int64_t value);

/*
 * Host-only helper, no GPU needed: edges-to-root for every node and the
 * reference's `depth` (MuchTree.pyx:218-225).  out_depths may be NULL.
 */
int st_host_depths(const int32_t *parent, int64_t n_nodes, int32_t *out_depths,
                   int32_t *out_tree_depth);

/*
 * Host-only helper, no GPU needed: the link-pair draws of SuchLinkedTrees.sample_linked_distances
 * (SuchTree/MuchTree.pyx:3025-3038) with the reference's own generator, xorshift64* (`_random_int`, :2937-2949:
 * state ^= state >> 12; state ^= state << 25; state ^= state >> 27; draw = (state * 2685821657736338717) % n_links).
 * For each of `count` samples two draws l1, l2 in that order; query_a[k] = (linklist[l1][1], linklist[l2][1]),
 * query_b[k] = (linklist[l1][0], linklist[l2][0]); `linklist` is (n_links, 2) int64, row-major.  `state` is read and
 * left at the generator's state after the last draw, so consecutive calls continue one sequence.
 */
int st_link_sample_pairs(uint64_t *state, const int64_t *linklist, int64_t n_links, int64_t count,
                         int64_t *query_a, int64_t *query_b);

/*
 * Host-only helper: the per-bucket running moments of sample_linked_distances (SuchTree/MuchTree.pyx:3044-3048 as
 * compiled, SuchTree/MuchTree.c:65197-65242): for i < buckets, j < n in that order
 * sums[i] += dist[i * n + j]; sumsq[i] += pow(dist[i * n + j], 2.0) -- doubles, the C library's pow.
 */
int st_bucket_moments(const double *dist, int64_t buckets, int64_t n, double *sums, double *sumsq);

/*
 * Native Newick ingest (host only).  Replaces the dendropy calls of SuchTree.__init__
 * (SuchTree/MuchTree.pyx:138-157, 171-216): first tree of the text, polytomies resolved,
 * nodes numbered in order.  st_newick_open parses and reports sizes; st_newick_fill copies
 * the flat arrays (any pointer may be NULL) -- leaf names come back concatenated, in
 * increasing leaf-id order, with n_leaves+1 byte offsets; st_newick_close frees.
 * ST_ERR_TREE means "not handled here" (syntax error or a token whose Python meaning is
 * not reproduced): callers fall back to suchtree_amd/newick.py, which owns the errors.
 */
typedef struct st_newick st_newick;
int st_newick_open(const char *text, int64_t len, st_newick **out, int64_t *n_nodes,
                   int64_t *n_leaves, int64_t *names_bytes, int32_t *root, int32_t *depth);
int st_newick_fill(const st_newick *h, int32_t *parent, int32_t *left, int32_t *right,
                   float *support, float *distance, int32_t *leaf_ids, char *names,
                   int64_t *name_offsets);
void st_newick_close(st_newick *h);

/* Thin device-memory helpers so callers without torch can stage buffers. */
int st_device_malloc(int device, int64_t bytes, void **out);
int st_device_free(int device, void *ptr);
int st_memcpy_h2d(int device, void *dst, const void *src, int64_t bytes);
int st_memcpy_d2h(int device, void *dst, const void *src, int64_t bytes);
int st_device_synchronize(int device);

#ifdef __cplusplus
}
#endif
#endif /* SUCHTREE_HIP_H */
