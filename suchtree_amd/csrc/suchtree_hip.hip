// suchtree_hip.hip -- gfx950 kernels and the C ABI of libsuchtree_hip.so.
//
// Hot path replaced: SuchTree._distances + SuchTree._mrca
// (/root/reference/SuchTree/MuchTree.pyx:911-943, 999-1030).  One wavefront
// lane per node pair.  Two kernel families, bit-identical results:
//
//   walk    pointer chase over the 8-byte {parent,dist} table with a depth
//           cut; works for any rooted tree.
//   canopy  the top of the tree lives in LDS (BFS-numbered); everything below it is
//           folded into one fixed-stride understory record per node (split into an
//           8-byte a-side table and a b-side table), so a pair costs two record reads
//           plus an LDS climb instead of ~h dependent global gathers.
//           k_canopy_ilp     one pair per lane, predicated (shallow canopies: the default)
//           k_canopy_ladder  deep canopies, large batches, long records: records read once, chain in
//                            registers, meeting node from a sparse table, both sides climbed on the
//                            ladder form of the canopy (three edges per 16-byte LDS entry)
//           k_canopy_sorted  deep canopies: pairs sorted by climb length within a workgroup tile; with
//                            in-order ids the meeting node comes from a sparse table and a's side from
//                            per-node lineage sums
//
// Every kernel is templated on a pair source (SrcContig / SrcContig32 / SrcStrided /
// SrcTriangle / SrcGrid / SrcQuartet): an explicit (n,2) array, or pairs derived from their
// index (all-pairs triangle, rows x columns grid, the six pairs of a quartet).
//
// Four translation units (compiled in parallel, build.py): launch_walk.hip (kernels_walk.h), launch_canopy.hip
// (kernels_canopy.h), launch_canopy_sorted.hip (kernels_canopy_sorted.h) -- each a kernel family with its launch
// functions, exported through launch_decl.h -- and this file: error plumbing and the C ABI, each export its argument
// checks, the device scope, at most a plan call and one call into the host side, which lives in the headers included below:
// st_tree.h / host_tree.h (handle, pipe registry), device_res.h (the owners of device and pinned memory, streams
// and events that the handle and the host calls hold), launch_policy.h + host_launch.h (which family a request gets,
// enqueueing, faults), host_upload.h (tables -> device),
// host_options.h (the handle options of st_tree_set_option: one table, one setter),
// host_path.h (host-buffer pipeline, mailbox, copy kernels; the one staged run behind st_distances_host[_i32], st_triangle_host, st_grid_host),
// host_misc.h (the drivers of kernels_misc.h: 24-bit id unpack, k nearest, graph matrices),
// and the compare paths (st_compare_*: two trees' distances over the same
// pairs, reduced on the device): kernels_compare.h / kernels_clades.h / kernels_rows.h (moments and 2-D histogram, clade
// pieces, row blocks), host_compare.h (TwoTreeSession, ReadbackRing, the chunk driver compare_run and its reducers, the pair
// inputs, statistics and the one skeleton, compare_entry, of the triangle / pairs entry points; clades_run and rows_run) and,
// host-only C++ beside tree_prep.cpp, compare_plan.cpp (argument checks, clade plan and tables, rows layout, the fold);
// plan_checks.h is what the plan units share in their checks (how one fails, a table of position sets, a range of the
// triangle of set pairs and that triangle's index, which the kernels share).
// Exact Spearman rank sums of the same pairs (st_compare_*_ranks_host): kernels_ranks.h, the reducers at the end of
// host_compare.h and, host-only, rank_plan.cpp (keys, bucket layout, tie arithmetic, st_spearman_host).
// Exact Kendall tau-b counts of the same pairs (st_compare_*_kendall_host, st_kendall_arrays_host): kernels_kendall.h (keys,
// tile sort, merge levels, tie scans), KendallState and its reducer at the end of host_compare.h and, host-only,
// kendall_plan.cpp (the merge arithmetic both sides share, st_kendall_host).
// Two trees' quartet topologies, counted on the device (st_compare_quartets_*_host, st_quartet_positions):
// kernels_quartets.h (generator, classify-and-count), host_quartets.h (the chunk driver; quartets_host_run, one tree's
// topologies through its own pipe: st_quartets_host) and, host-only,
// quartet_plan.cpp (unranking, the draw, the class rule, argument checks).
// The keyed permutation behind every null (st_hommola_permutation): keyed_perm.h (key, size classes, the host form; host
// and device) and kernels_perm.h (the device sort).  Hommola's permutation test for many clades at once
// (st_hommola_clades_host): kernels_hommola.h (the sorts that relabel the links, the blocks over two distance matrices),
// host_hommola.h (the chunk driver) and, host-only, hommola_plan.cpp (argument checks, ranges, block and chunk tables, the fold).
// MPD / MNTD sums of many leaf sets under the taxa-labels null (st_partner_dispersion_host, st_dispersion_matrix):
// kernels_dispersion.h (one sort per permutation, the k x k reducer in three size classes), host_dispersion.h (the chunk
// drivers) and, host-only, dispersion_plan.cpp (argument checks, size classes, chunks, the restatement of the reduction).
// The same sums under the degree-preserving swap null (st_swap_null_tables, st_dispersion_matrix_swap,
// st_partner_dispersion_swap_host): kernels_swap.h (one wave per Markov chain of swaps), the table form of kernels_dispersion.h's
// reducers, host_swap.h (the block of chains, the chunk loop with the chains as its producer) and, host-only, swap_plan.cpp.
// betaMPD / betaMNTD sums between every two leaf sets under the same null (st_beta_dispersion_host, st_beta_dispersion_matrix):
// kernels_setpair.h (the k_r x k_c reducer in the same three size classes), host_dispersion.h (one launcher, chunk driver,
// tree run and matrix run for both passes) and, host-only, setpair_plan.cpp (argument checks, the task table, the restatement).
// Faith's PD of many leaf sets and the union sums of their pairs behind UniFrac (st_unifrac_host, st_unifrac_depths):
// kernels_unifrac.h (the range-minimum table, the set merge in a lane form and a wave form), host_unifrac.h (the depths, the
// chunk driver) and, host-only, unifrac_plan.cpp (argument checks, the quantiser, chunks, the restatement of the merge).
// The same sums under the taxa-labels null (st_unifrac_null_host, st_unifrac_null_depths): kernels_unifrac_null.h (the
// relabelling of every set under every shuffle through an LDS bitmap, the pair kernels over the relabelled table),
// host_unifrac_null.h (its part of the work block and its launches; the head of the block and the depths are
// host_unifrac.h's, the loop over blocks and chunks host_dispersion.h's) and, host-only, unifrac_null_plan.cpp (checks, layout, restatement).
// Every induced clade of one tree matched to the closest of another's, behind Robinson-Foulds and transfer support
// (st_clade_ranges, st_clade_match): kernels_clade_match.h (a bitmap and running counts in LDS, one row per workgroup),
// host_clade_match.h (the chunk driver) and, host-only, clade_match_plan.cpp (the range builder, the checks, the size
// windows, the restatement).
// The Mantel and partial Mantel sums of two or three distance matrices under the same relabelling null (st_mantel_codes,
// st_mantel_quantise): kernels_mantel.h (a wave form with the matrix in LDS, a row form that stages one matrix row in LDS
// per workgroup, the fold), host_mantel.h (the layout, the launches) and, host-only, mantel_plan.cpp (the checks, the
// invariant sums, the quantiser, the restatement).  This and the next three are the matrix permutation tests: their plans
// derive from MatrixPlan and are cut by dispersion_cut_blocks (dispersion_plan.cpp), their device sides open the work block
// and walk blocks and chunks with host_dispersion.h's open_work_block and matrix_block_chunks.
// The within-group sums of a distance matrix under the same relabelling null, behind PERMANOVA and ANOSIM
// (st_group_sums_codes): kernels_group.h (a wave form with y in LDS; the relabelled labels as bytes, a row form that
// stages a row of y in LDS once for a slice of permutations, the fold by group), host_group.h (the layout, the launches) and, host-only,
// group_plan.cpp (the checks, the layout, the restatement).
// The per-class sums of a distance matrix under the same relabelling null, behind the Mantel correlogram
// (st_class_sums_codes): kernels_class.h (the class square expanded once, a wave form with y and the square in LDS, a row
// form that stages a row pair of y in LDS once for a slice of permutations and files each pair under its class in LDS
// accumulators, the fold), host_class.h (the layout, the launches) and, host-only, class_plan.cpp (the checks,
// the layout, the restatement).
// ParaFit's global statistic and ParaFitLink1 of every host-guest link as exact sums over link pairs (st_parafit_codes):
// kernels_parafit.h (the held side expanded once, one sort per permutation and linked leaf, a wave form with both sides in
// LDS, a row form that stages one matrix row in LDS per workgroup, the fold with the per-link counts), host_parafit.h (the
// layout, the launches) and, host-only, parafit_plan.cpp (the checks, the layout, the restatement).
// Exact UPGMA, single and complete linkage of a matrix of codes (st_linkage_codes): kernels_linkage.h (the square of pair
// sums, every row's nearest later partner, the chain of merges as one workgroup), host_linkage.h (the layout, the three
// launches, where the cache lives) and, host-only, linkage_plan.cpp (the checks, the restatement with the same cache).
// The clades a whole set of trees shares, pair by pair (st_rf_tasks): kernels_rf.h (Day's method, one task per workgroup:
// a scatter, block extrema and a sparse table in LDS, a binary search per clade), host_rf.h (the work block and the chunk
// driver) and, host-only, rf_plan.cpp (the checks, the sorted keys, the restatement of the method).
//
// What the host side does: tree upload to one or several GPUs (tree_prep.cpp builds the tables, under a table budget
// if one is given), the host path (host_pipe.h, host_copy.h: packed ids in through the copy engine, kernels write
// float32 + 24-bit ids straight into pinned host memory), the small-batch mailbox, fault read-back, the creation-time
// choice of a deep tree's kernels (host_tune.h).
//
// Built for gfx950 only: hipcc --offload-arch=gfx950 -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/suchtree_hip.h"
#include "host_copy.h"
#include "host_pipe.h"
#include "pair_math.h"
#include "tree_prep.h"

namespace st {

// --------------------------------------------------------------------------
// error plumbing
// --------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

// Nothing may be thrown through the C ABI (the callers are ctypes, cgo, JNI ...): every int-returning export is
// a function-try-block that ends in ST_CATCH_ALL.
static int on_exception() noexcept
{
    try {
        throw;
    } catch (const std::bad_alloc &) {
        try { g_last_error = "out of host memory"; } catch (...) {}
        return ST_ERR_NOMEM;
    } catch (const std::exception &e) {
        try { g_last_error = std::string("internal error: ") + e.what(); } catch (...) {}
        return ST_ERR_HIP;
    } catch (...) {
        try { g_last_error = "internal error"; } catch (...) {}
        return ST_ERR_HIP;
    }
}
#define ST_CATCH_ALL catch (...) { return st::on_exception(); }

#define ST_HIP(call)                                                              \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess)                                                     \
            return fail(ST_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Selects a device for the scope of one C-ABI call and puts the caller's current device
// back afterwards (callers such as PyTorch keep their own notion of "current device").
class DeviceScope {
public:
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        err_ = (prev_ == device) ? hipSuccess : hipSetDevice(device);
        changed_ = err_ == hipSuccess && prev_ != device;
    }
    ~DeviceScope()
    {
        if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    hipError_t error() const { return err_; }

private:
    int prev_ = -1;
    hipError_t err_ = hipSuccess;
    bool changed_ = false;
};

#define ST_DEVICE(dev)                                                                     \
    DeviceScope device_scope_(dev);                                                        \
    if (device_scope_.error() != hipSuccess)                                               \
        return fail(ST_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_scope_.error()))

// the `device` of a call that also has a host form
static int device_or_host_arg(int device) { return device < -1 ? fail(ST_ERR_ARG, "device must be -1 (host) or a device index") : ST_OK; }

static int device_index_arg(int device)
{
    int n_dev = 0;
    ST_HIP(hipGetDeviceCount(&n_dev));
    if (device >= n_dev) return fail(ST_ERR_ARG, "device " + std::to_string(device) + " of " + std::to_string(n_dev));
    return ST_OK;
}

}  // namespace st

#include "device_common.h"
#include "kernels_misc.h"
#include "kernels_compare.h"
#include "kernels_ranks.h"
#include "kernels_kendall.h"
#include "kernels_clades.h"
#include "kernels_rows.h"
#include "kernels_quartets.h"
#include "kernels_perm.h"
#include "kernels_hommola.h"
#include "kernels_dispersion.h"
#include "kernels_swap.h"
#include "kernels_setpair.h"
#include "kernels_unifrac.h"
#include "kernels_unifrac_null.h"
#include "kernels_clade_match.h"
#include "kernels_mantel.h"
#include "kernels_group.h"
#include "kernels_class.h"
#include "kernels_parafit.h"
#include "kernels_linkage.h"
#include "kernels_rf.h"


// --------------------------------------------------------------------------
// host side: the tree handle
// --------------------------------------------------------------------------
using namespace st;

#include "host_tree.h"
#include "host_options.h"
#include "host_launch.h"
#include "host_path.h"
#include "host_misc.h"
#include "host_tune.h"
#include "host_upload.h"
#include "host_compare.h"
#include "host_quartets.h"
#include "host_hommola.h"
#include "host_dispersion.h"
#include "host_swap.h"
#include "host_unifrac.h"
#include "host_unifrac_null.h"
#include "host_clade_match.h"
#include "host_mantel.h"
#include "host_group.h"
#include "host_class.h"
#include "host_parafit.h"
#include "host_linkage.h"
#include "host_rf.h"

// the next link of st_link_sample_pairs (MuchTree.pyx:2946-2949)
static int64_t link_draw(uint64_t &s, int64_t n_links)
{
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (int64_t)((s * 2685821657736338717ull) % (uint64_t)n_links);
}

extern "C" {

const char *st_last_error(void) { return g_last_error.c_str(); }

int st_device_count(int *count)
try {
    if (!count) return fail(ST_ERR_ARG, "count is NULL");
    *count = 0;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ST_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = c;
    return ST_OK;
} ST_CATCH_ALL

int st_host_depths(const int32_t *parent, int64_t n_nodes, int32_t *out_depths, int32_t *out_tree_depth)
try {
    if (!parent || n_nodes <= 0) return fail(ST_ERR_ARG, "parent is NULL or n_nodes <= 0");
    std::vector<float> zeros((size_t)n_nodes, 0.0f);
    TreeTables T;
    std::string err;
    if (!prepare_basic(parent, zeros.data(), n_nodes, T, err)) return fail(ST_ERR_TREE, err);
    if (out_depths) std::memcpy(out_depths, T.depth.data(), (size_t)n_nodes * 4);
    if (out_tree_depth) *out_tree_depth = T.tree_depth;
    return ST_OK;
} ST_CATCH_ALL

int st_link_sample_pairs(uint64_t *state, const int64_t *linklist, int64_t n_links, int64_t count, int64_t *query_a,
                         int64_t *query_b)
try {
    if (!state || !linklist || n_links < 1 || count < 0 || (count > 0 && (!query_a || !query_b)))
        return fail(ST_ERR_ARG, "state / linklist / query arrays are NULL, n_links < 1 or count < 0");
    uint64_t s = *state;
    for (int64_t k = 0; k < count; k++) {
        const int64_t l1 = link_draw(s, n_links), l2 = link_draw(s, n_links);
        query_a[2 * k] = linklist[2 * l1 + 1];
        query_a[2 * k + 1] = linklist[2 * l2 + 1];
        query_b[2 * k] = linklist[2 * l1];
        query_b[2 * k + 1] = linklist[2 * l2];
    }
    *state = s;
    return ST_OK;
} ST_CATCH_ALL

int st_bucket_moments(const double *dist, int64_t buckets, int64_t n, double *sums, double *sumsq)
try {
    if (buckets < 0 || n < 0 || (buckets > 0 && n > 0 && (!dist || !sums || !sumsq)))
        return fail(ST_ERR_ARG, "dist / sums / sumsq are NULL or a size is negative");
    for (int64_t i = 0; i < buckets; i++)
        for (int64_t j = 0; j < n; j++) {
            const double d = dist[i * n + j];
            sums[i] += d;
            sumsq[i] += std::pow(d, 2.0);
        }
    return ST_OK;
} ST_CATCH_ALL

int st_host_chunk_plan(int64_t n, int n_devices, int64_t *chunk_pairs, int64_t *n_chunks)
try {
    if (n < 0 || n_devices < 1) return fail(ST_ERR_ARG, "n < 0 or n_devices < 1");
    const int64_t chunk = host_chunk_pairs(n, n_devices);
    if (chunk_pairs) *chunk_pairs = chunk;
    if (n_chunks) *n_chunks = (n + chunk - 1) / chunk;
    return ST_OK;
} ST_CATCH_ALL

int st_host_chunk_owner(int64_t n, int n_devices, int64_t chunk_index, int *device_index,
                        int64_t *first_pair, int64_t *n_pairs)
try {
    if (n < 0 || n_devices < 1 || chunk_index < 0) return fail(ST_ERR_ARG, "bad arguments");
    const int64_t chunk = host_chunk_pairs(n, n_devices);
    if (chunk_index * chunk >= n) return fail(ST_ERR_ARG, "chunk index past the end of the batch");
    // the same arithmetic as ChunkSeq / run_pipe
    if (device_index) *device_index = (int)(chunk_index % n_devices);
    if (first_pair) *first_pair = chunk_index * chunk;
    if (n_pairs) *n_pairs = std::min(chunk, n - chunk_index * chunk);
    return ST_OK;
} ST_CATCH_ALL

static int check_create_args(const int32_t *parent, const float *distance, int64_t n_nodes, int strategy, st_tree **out)
{
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!parent || !distance || n_nodes <= 0) return fail(ST_ERR_ARG, "parent/distance NULL or n_nodes <= 0");
    if (strategy != ST_STRATEGY_AUTO && strategy != ST_STRATEGY_WALK && strategy != ST_STRATEGY_CANOPY)
        return fail(ST_ERR_ARG, "unknown strategy " + std::to_string(strategy));
    return ST_OK;
}

int st_tree_create(const int32_t *parent, const float *distance, int64_t n_nodes, int device,
                   int strategy, st_tree **out)
try {
    int rc = check_create_args(parent, distance, n_nodes, strategy, out);
    if (rc != ST_OK) return rc;
    BuiltTables B;
    rc = build_tables(parent, distance, n_nodes, strategy, B);
    if (rc != ST_OK) return rc;
    return upload_tree(B, device, out);
} ST_CATCH_ALL

static int create_multi(const int32_t *parent, const float *distance, int64_t n_nodes, const int *devices, int n_devices,
                        int strategy, int64_t budget_option, st_tree **out);

int st_tree_create_multi(const int32_t *parent, const float *distance, int64_t n_nodes,
                         const int *devices, int n_devices, int strategy, st_tree **out)
try {
    return create_multi(parent, distance, n_nodes, devices, n_devices, strategy, 0, out);
} ST_CATCH_ALL

int st_tree_create_ex(const int32_t *parent, const float *distance, int64_t n_nodes, const int *devices, int n_devices,
                      int strategy, const st_tree_options *opts, st_tree **out)
try {
    if (opts && opts->table_budget_bytes < 0) return fail(ST_ERR_ARG, "table_budget_bytes < 0");
    return create_multi(parent, distance, n_nodes, devices, n_devices, strategy, opts ? opts->table_budget_bytes : 0, out);
} ST_CATCH_ALL

int st_host_table_plan(const int32_t *parent, const float *distance, int64_t n_nodes, int strategy, int64_t table_budget_bytes,
                       int64_t *device_bytes, int32_t *dropped_tables, int32_t *family)
try {
    st_tree *unused = nullptr;
    int rc = check_create_args(parent, distance, n_nodes, strategy, &unused);
    if (rc != ST_OK) return rc;
    if (table_budget_bytes < 0) return fail(ST_ERR_ARG, "table_budget_bytes < 0");
    BuiltTables B;
    rc = build_tables(parent, distance, n_nodes, strategy, B, table_budget_bytes);
    if (rc != ST_OK) return rc;
    if (device_bytes) *device_bytes = device_bytes_of(B);
    if (dropped_tables) *dropped_tables = B.dropped;
    if (family) *family = B.canopy_ok ? ST_STRATEGY_CANOPY : ST_STRATEGY_WALK;
    return ST_OK;
} ST_CATCH_ALL

}  // extern "C"

static int create_multi(const int32_t *parent, const float *distance, int64_t n_nodes, const int *devices, int n_devices,
                        int strategy, int64_t budget_option, st_tree **out)
{
    int rc = check_create_args(parent, distance, n_nodes, strategy, out);
    if (rc != ST_OK) return rc;
    if (!devices || n_devices < 1) return fail(ST_ERR_ARG, "devices is NULL or n_devices < 1");
    // (SUCHTREE_AMD_ALLOW_DUPLICATE_DEVICES=1: testing aid -- several replicas on one GPU, so that
    // the dealing of chunks over replicas can run on a single-GPU box; they take turns on its pipe)
    const char *dup = std::getenv("SUCHTREE_AMD_ALLOW_DUPLICATE_DEVICES");
    if (!dup || dup[0] != '1')
        for (int i = 0; i < n_devices; i++)
            for (int j = 0; j < i; j++)
                if (devices[i] == devices[j]) return fail(ST_ERR_ARG, "device " + std::to_string(devices[i]) + " listed twice");
    BuiltTables B;
    rc = build_tables(parent, distance, n_nodes, strategy, B, budget_option);
    if (rc != ST_OK) return rc;
    st_tree *primary = nullptr;
    rc = upload_tree(B, devices[0], &primary);
    if (rc != ST_OK) return rc;
    TreeOwner owner{primary};      // (destroys the primary and the peers it holds unless every replica was built)
    primary->peers.reserve((size_t)n_devices);
    for (int i = 1; i < n_devices; i++) {
        st_tree *peer = nullptr;
        rc = upload_tree(B, devices[i], &peer, false);
        if (rc != ST_OK) return rc;
        if (B.deep) copy_tuned_settings(peer, primary);      // one measurement per handle: every replica runs the same kernel
        primary->peers.push_back(peer);
    }
    primary->info.n_devices = n_devices;
    owner.t = nullptr;
    *out = primary;
    return ST_OK;
}

extern "C" {

void st_tree_destroy(st_tree *t)
{
    if (!t) return;
    for (st_tree *p : t->peers) st_tree_destroy(p);
    t->peers.clear();
    const int device = t->device;
    const bool has_pipe = t->dp != nullptr;
    {
        DeviceScope scope(device);      // (the handle's owners release their memory, events and stream on its device)
        delete t;
    }
    if (has_pipe) pipe_release(device);
}

int st_tree_info_get(const st_tree *t, st_tree_info *info)
try {
    if (!t || !info) return fail(ST_ERR_ARG, "tree or info is NULL");
    *info = t->info;
    info->strategy = t->strategy;
    info->big_batch_kernel = big_batch_kernel_of(t);      // (follows the handle's current options)
    info->heap_lines = heap_lines_applies(t) ? 1 : 0;
    info->heap_codes = heap_codes_applies(t, (int64_t)1 << 40) ? 1 : 0;      // (large batches: the same launches from the table of 20-bit codes; nothing below follows it)
    info->stream_hint = stream_hint_applies(t, (int64_t)1 << 40, true) ? 1 : 0;      // (large explicit batches with distances)
    info->a_side_bytes = t->has_canopy ? ((info->heap_lines || (t->rec_a4 && t->d_rec_a4 && t->d_leaf_blocks)) ? 4 : 8) : 0;
    // (heap lines: both nodes of a pair gather from the one table of 8 bytes per leaf -- 4 + 4)
    info->b_table_bytes_per_leaf = info->heap_lines ? 4 : t->has_canopy ? ((t->rec_a4 && t->cherries && t->d_rec_c && t->d_leaf_blocks) ? t->rec_bytes / 4 : t->rec_bytes / 2) : 0;
    info->ladder_sums = (t->ladder_sums && ladder_sums_ready(t)) ? 1 : 0;      // (for batches of up to ladder_sums_max_pairs, if that is set)
    info->ladder_sums_max_pairs = info->ladder_sums ? t->ladder_sums_max_pairs : 0;
    info->host_wire_bytes_in = t->wire48 && t->n_nodes <= 0xFFFFFF ? 6 : 8;
    info->host_wire_bytes_out = t->wire24 && t->n_nodes <= 0xFFFFFF ? 7 : 8;
    return ST_OK;
} ST_CATCH_ALL

int st_api_version(void) { return ST_API_VERSION; }

int st_tree_info_get_sized(const st_tree *t, void *info, int64_t info_bytes)
try {
    if (!t || !info) return fail(ST_ERR_ARG, "tree or info is NULL");
    if (info_bytes < 8 || info_bytes % 4) return fail(ST_ERR_ARG, "info_bytes must be a multiple of 4, at least 8");
    st_tree_info full;
    const int rc = st_tree_info_get(t, &full);
    if (rc != ST_OK) return rc;
    std::memcpy(info, &full, (size_t)std::min<int64_t>(info_bytes, (int64_t)sizeof full));
    return ST_OK;
} ST_CATCH_ALL

int st_tree_devices(const st_tree *t, int *devices, int capacity, int *n_devices)
try {
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    const int n = 1 + (int)t->peers.size();
    if (n_devices) *n_devices = n;
    if (devices)
        for (int i = 0; i < n && i < capacity; i++) devices[i] = i == 0 ? t->device : t->peers[(size_t)i - 1]->device;
    return ST_OK;
} ST_CATCH_ALL

int st_tree_set_strategy(st_tree *t, int strategy)
try {
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    if (strategy == ST_STRATEGY_AUTO) strategy = t->has_canopy ? ST_STRATEGY_CANOPY : ST_STRATEGY_WALK;
    if (strategy == ST_STRATEGY_CANOPY && !t->has_canopy)
        return fail(ST_ERR_ARG, "tree was built without canopy tables");
    if (strategy != ST_STRATEGY_CANOPY && strategy != ST_STRATEGY_WALK)
        return fail(ST_ERR_ARG, "unknown strategy " + std::to_string(strategy));
    t->strategy = strategy;
    for (st_tree *p : t->peers) p->strategy = strategy;
    return ST_OK;
} ST_CATCH_ALL

int st_tree_set_option(st_tree *t, const char *name, int64_t value)
try {
    if (!t || !name) return fail(ST_ERR_ARG, "tree or name is NULL");
    int rc = set_option_one(t, name, value);
    for (st_tree *p : t->peers)
        if (rc == ST_OK) rc = set_option_one(p, name, value);
    return rc;
} ST_CATCH_ALL

// what every entry over explicit pairs checks first, in this order (host and device forms)
static int pair_batch_args(const st_tree *t, const void *pairs, int64_t n, const void *out_d, const void *out_m)
{
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    if (n < 0) return fail(ST_ERR_ARG, "n < 0");
    if (n > 0 && !pairs) return fail(ST_ERR_ARG, "pairs is NULL");
    if (!out_d && !out_m) return fail(ST_ERR_ARG, "both outputs are NULL");
    return ST_OK;
}

int st_distances_device(st_tree *t, const int64_t *d_pairs, int64_t n, int64_t stride0,
                        int64_t stride1, double *d_out_dist, int32_t *d_out_mrca, void *stream)
try {
    const int rc = pair_batch_args(t, d_pairs, n, d_out_dist, d_out_mrca);
    if (rc != ST_OK) return rc;
    ST_DEVICE(t->device);
    return enqueue(t, d_pairs, n, stride0, stride1, DistSink{d_out_dist, nullptr}, MrcaSink{d_out_mrca, nullptr},
                   reinterpret_cast<hipStream_t>(stream));
} ST_CATCH_ALL

int st_distances_device_f32(st_tree *t, const int64_t *d_pairs, int64_t n, int64_t stride0,
                            int64_t stride1, float *d_out_dist, int32_t *d_out_mrca, void *stream)
try {
    const int rc = pair_batch_args(t, d_pairs, n, d_out_dist, d_out_mrca);
    if (rc != ST_OK) return rc;
    ST_DEVICE(t->device);
    return enqueue(t, d_pairs, n, stride0, stride1, DistSink{nullptr, d_out_dist}, MrcaSink{d_out_mrca, nullptr},
                   reinterpret_cast<hipStream_t>(stream));
} ST_CATCH_ALL

int st_distances_device_wire(st_tree *t, const int64_t *d_pairs, int64_t n, int64_t stride0, int64_t stride1,
                             float *d_out_dist, uint8_t *d_out_mrca24, void *stream)
try {
    const int rc = pair_batch_args(t, d_pairs, n, d_out_dist, d_out_mrca24);
    if (rc != ST_OK) return rc;
    if (t->n_nodes > 0xFFFFFF) return fail(ST_ERR_ARG, "24-bit MRCA ids need a tree of fewer than 2^24 nodes");
    if (reinterpret_cast<uintptr_t>(d_out_mrca24) & 3) return fail(ST_ERR_ARG, "d_out_mrca24 must be 4-byte aligned");
    ST_DEVICE(t->device);
    return enqueue(t, d_pairs, n, stride0, stride1, DistSink{nullptr, d_out_dist}, MrcaSink{nullptr, d_out_mrca24},
                   reinterpret_cast<hipStream_t>(stream));
} ST_CATCH_ALL

int st_unpack_mrca24_device(int device, const uint8_t *d_packed, int64_t n, int32_t *d_out_mrca, void *stream)
try {
    if (n < 0) return fail(ST_ERR_ARG, "n < 0");
    if (n == 0) return ST_OK;
    if (!d_packed || !d_out_mrca) return fail(ST_ERR_ARG, "buffer is NULL");
    return unpack_mrca24_run(device, d_packed, n, d_out_mrca, stream);
} ST_CATCH_ALL

int st_fault_check(st_tree *t, void *stream, int64_t *bad_id)
try {
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    ST_DEVICE(t->device);
    Fault f;
    const int rc = fetch_fault(t->d_fault, reinterpret_cast<hipStream_t>(stream), f);
    if (rc != ST_OK) return rc;
    return report_fault(t->n_nodes, f, bad_id);
} ST_CATCH_ALL

int st_probe_last_choice(st_tree *t, void *stream, int *choice)
try {
    if (!t || !choice) return fail(ST_ERR_ARG, "tree or choice is NULL");
    *choice = -1;
    const unsigned issued = t->choice_next.load(std::memory_order_relaxed);
    if (!t->d_choice || issued == 0) return ST_OK;
    ST_DEVICE(t->device);
    ST_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    ST_HIP(hipMemcpy(choice, t->d_choice + (issued - 1) % kWorkSlots, sizeof(int), hipMemcpyDeviceToHost));
    return ST_OK;
} ST_CATCH_ALL

int st_distances_host(st_tree *t, const int64_t *pairs, int64_t n, int64_t stride0, int64_t stride1,
                      double *out_dist, int32_t *out_mrca, int64_t *bad_id)
try {
    const int rc = pair_batch_args(t, pairs, n, out_dist, out_mrca);
    if (rc != ST_OK || n == 0) return rc;
    return distances_host_run(t, pairs, n, stride0, stride1, out_dist, out_mrca, bad_id);
} ST_CATCH_ALL

int st_distances_host_i32(st_tree *t, const int32_t *pairs, int64_t n, int64_t stride0, int64_t stride1,
                          double *out_dist, int32_t *out_mrca, int64_t *bad_id)
try {
    const int rc = pair_batch_args(t, pairs, n, out_dist, out_mrca);
    if (rc != ST_OK || n == 0) return rc;
    return distances_host_run(t, pairs, n, stride0, stride1, out_dist, out_mrca, bad_id);
} ST_CATCH_ALL

static int triangle_args(st_tree *t, const int64_t *ids, int64_t m, int64_t k_begin, int64_t k_count,
                         const void *out_d, const void *out_m)
{
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    const int rc = triangle_range_args(m, k_begin, k_count);
    if (rc != ST_OK) return rc;
    if (k_count > 0 && !ids) return fail(ST_ERR_ARG, "ids is NULL");
    if (!out_d && !out_m) return fail(ST_ERR_ARG, "both outputs are NULL");
    return ST_OK;
}

int st_triangle_device(st_tree *t, const int64_t *d_ids, int64_t m, int64_t id_stride,
                       int64_t k_begin, int64_t k_count, double *d_out_dist, int32_t *d_out_mrca,
                       void *stream)
try {
    int rc = triangle_args(t, d_ids, m, k_begin, k_count, d_out_dist, d_out_mrca);
    if (rc != ST_OK) return rc;
    ST_DEVICE(t->device);
    const SrcTriangle src{reinterpret_cast<const long long *>(d_ids), (long long)id_stride, (long long)k_begin};
    return enqueue_src(t, src, k_count, DistSink{d_out_dist, nullptr}, MrcaSink{d_out_mrca, nullptr}, t->d_fault,
                       reinterpret_cast<hipStream_t>(stream));
} ST_CATCH_ALL

int st_triangle_host(st_tree *t, const int64_t *ids, int64_t m, int64_t id_stride, int64_t k_begin,
                     int64_t k_count, double *out_dist, int32_t *out_mrca, int64_t *bad_id)
try {
    const int rc = triangle_args(t, ids, m, k_begin, k_count, out_dist, out_mrca);
    if (rc != ST_OK || k_count == 0) return rc;
    return triangle_host_run(t, ids, m, id_stride, k_begin, k_count, out_dist, out_mrca, bad_id);
} ST_CATCH_ALL

static int grid_args(st_tree *t, const int64_t *rows, int64_t n_rows, const int64_t *cols, int64_t n_cols,
                     int64_t e_begin, int64_t e_count, const void *out_d, const void *out_m)
{
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    if (n_rows < 0 || n_cols < 0 || e_begin < 0 || e_count < 0) return fail(ST_ERR_ARG, "negative size");
    if (n_rows > 3000000000LL || n_cols > 3000000000LL) return fail(ST_ERR_ARG, "grid too large");
    if (e_begin + e_count > n_rows * n_cols) return fail(ST_ERR_ARG, "element range exceeds n_rows * n_cols");
    if (e_count > 0 && (!rows || !cols)) return fail(ST_ERR_ARG, "id list is NULL");
    if (!out_d && !out_m) return fail(ST_ERR_ARG, "both outputs are NULL");
    return ST_OK;
}

int st_grid_host(st_tree *t, const int64_t *row_ids, int64_t n_rows, const int64_t *col_ids, int64_t n_cols,
                 int symmetric, int64_t e_begin, int64_t e_count, double *out_dist, int32_t *out_mrca,
                 int64_t *bad_id)
try {
    const int rc = grid_args(t, row_ids, n_rows, col_ids, n_cols, e_begin, e_count, out_dist, out_mrca);
    if (rc != ST_OK) return rc;
    if (symmetric && (n_rows != n_cols)) return fail(ST_ERR_ARG, "symmetric grid needs n_rows == n_cols");
    if (e_count == 0) return ST_OK;
    return grid_host_run(t, row_ids, n_rows, col_ids, n_cols, symmetric, e_begin, e_count, out_dist, out_mrca, bad_id);
} ST_CATCH_ALL

int st_knn_host(st_tree *t, const int64_t *queries, int64_t n_queries, const int64_t *cands, int64_t n_cands,
                int k, int skip_self, int64_t *out_index, double *out_dist, int64_t *bad_id)
try {
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    if (n_queries < 0 || n_cands < 0) return fail(ST_ERR_ARG, "negative size");
    if (k < 1 || k > kKnnMaxK) return fail(ST_ERR_ARG, "k must be in [1, " + std::to_string(kKnnMaxK) + "]");
    if (n_cands > 0xFFFFFFFFLL) return fail(ST_ERR_ARG, "too many candidates");
    if (n_queries > 0 && (!queries || !out_index || !out_dist)) return fail(ST_ERR_ARG, "queries or output is NULL");
    if (n_cands > 0 && !cands) return fail(ST_ERR_ARG, "cands is NULL");
    if (n_queries == 0) return ST_OK;
    if (n_cands == 0) {
        for (int64_t i = 0; i < n_queries * k; i++) { out_index[i] = -1; out_dist[i] = std::numeric_limits<double>::quiet_NaN(); }
        return ST_OK;
    }
    return knn_host_run(t, queries, n_queries, cands, n_cands, k, skip_self, out_index, out_dist, bad_id);
} ST_CATCH_ALL

// ---- compare paths (st_compare_*_host, st_clade_plan) ---------------------------------------------------------------
// st_compare_{triangle,pairs}[_ranks|_kendall]_host are compare_entry (host_compare.h) over a pair input -- TriangleInput,
// PairsInput -- and a statistic -- MomentsStat, RanksStat, KendallStat: a new input or statistic is a struct there and one
// line here per entry point.

int st_compare_triangle_host(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t m, int64_t k_begin,
                             int64_t k_count, const double *edges_x, int32_t bins_x, const double *edges_y, int32_t bins_y,
                             st_pair_moments *out, int64_t *out_hist, int64_t *bad_id)
try {
    return compare_entry(tx, ty, TriangleInput{ids_x, ids_y, m, k_begin, k_count}, MomentsStat{edges_x, edges_y, bins_x, bins_y, out, out_hist},
                         bad_id);
} ST_CATCH_ALL

int st_compare_pairs_host(st_tree *tx, st_tree *ty, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n, const double *edges_x,
                          int32_t bins_x, const double *edges_y, int32_t bins_y, st_pair_moments *out, int64_t *out_hist,
                          int64_t *bad_id)
try {
    return compare_entry(tx, ty, PairsInput{pairs_x, pairs_y, n}, MomentsStat{edges_x, edges_y, bins_x, bins_y, out, out_hist}, bad_id);
} ST_CATCH_ALL

int st_compare_triangle_ranks_host(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t m, int64_t k_begin,
                                   int64_t k_count, int64_t chunk_pairs, st_pair_moments *out, st_rank_sums *out_ranks, int64_t *bad_id)
try {
    return compare_entry(tx, ty, TriangleInput{ids_x, ids_y, m, k_begin, k_count}, RanksStat{chunk_pairs, out, out_ranks}, bad_id);
} ST_CATCH_ALL

int st_compare_pairs_ranks_host(st_tree *tx, st_tree *ty, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n, int64_t chunk_pairs,
                                st_pair_moments *out, st_rank_sums *out_ranks, int64_t *bad_id)
try {
    return compare_entry(tx, ty, PairsInput{pairs_x, pairs_y, n}, RanksStat{chunk_pairs, out, out_ranks}, bad_id);
} ST_CATCH_ALL

int st_spearman_host(const float *x, const float *y, int64_t n, st_rank_sums *out)
try {
    std::string err;
    const int rc = spearman_host(x, y, n, out, err);
    return rc == ST_OK ? ST_OK : fail(rc, err);
} ST_CATCH_ALL

int st_compare_triangle_kendall_host(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t m, int64_t k_begin,
                                     int64_t k_count, int64_t chunk_pairs, st_pair_moments *out, st_kendall_counts *out_counts, int64_t *bad_id)
try {
    return compare_entry(tx, ty, TriangleInput{ids_x, ids_y, m, k_begin, k_count}, KendallStat{chunk_pairs, out, out_counts}, bad_id);
} ST_CATCH_ALL

int st_compare_pairs_kendall_host(st_tree *tx, st_tree *ty, const int64_t *pairs_x, const int64_t *pairs_y, int64_t n, int64_t chunk_pairs,
                                  st_pair_moments *out, st_kendall_counts *out_counts, int64_t *bad_id)
try {
    return compare_entry(tx, ty, PairsInput{pairs_x, pairs_y, n}, KendallStat{chunk_pairs, out, out_counts}, bad_id);
} ST_CATCH_ALL

int st_kendall_arrays_host(int device, const float *x, const float *y, int64_t n, st_kendall_counts *out)
try {
    std::string err;
    const int rc = kendall_args(x, y, n, out, err);
    if (rc != ST_OK) return fail(rc, err);
    if (n == 0) {
        kendall_finish(0, 0, 0, 0, 0, 0, out);
        return ST_OK;
    }
    return kendall_arrays(device, x, y, n, out);
} ST_CATCH_ALL

int st_kendall_host(const float *x, const float *y, int64_t n, st_kendall_counts *out)
try {
    std::string err;
    const int rc = kendall_host(x, y, n, out, err);
    return rc == ST_OK ? ST_OK : fail(rc, err);
} ST_CATCH_ALL

int st_clade_plan(const int32_t *parent, int64_t n_nodes, const int64_t *link_leaf, int64_t n_links, int64_t max_links,
                  int64_t *out_perm, int64_t *out_begin, int64_t *out_count, int64_t *out_leaves, st_clade_segment *out_segs,
                  int64_t seg_capacity, int64_t *out_n_segs, int64_t *out_total_pairs, int64_t *bad_id)
try {
    CladePlan P;
    std::string err;
    const int rc = clade_plan(parent, n_nodes, link_leaf, n_links, max_links, P, err);
    if (rc == ST_ERR_BOUNDS) return compare_check_ids(link_leaf, n_links, n_nodes, bad_id);      // (a second scan, to word it)
    if (rc != ST_OK) return fail(rc, err);
    if (out_segs && seg_capacity < (int64_t)P.segs.size())
        return fail(ST_ERR_ARG, "seg_capacity " + std::to_string(seg_capacity) + " < " + std::to_string(P.segs.size()) + " segments");
    if (out_perm) std::copy(P.perm.begin(), P.perm.end(), out_perm);
    if (out_begin) std::copy(P.begin.begin(), P.begin.end(), out_begin);
    if (out_count) std::copy(P.count.begin(), P.count.end(), out_count);
    if (out_leaves) std::copy(P.leaves.begin(), P.leaves.end(), out_leaves);
    if (out_segs) std::copy(P.segs.begin(), P.segs.end(), out_segs);
    if (out_n_segs) *out_n_segs = (int64_t)P.segs.size();
    if (out_total_pairs) *out_total_pairs = P.total;
    return ST_OK;
} ST_CATCH_ALL

int st_compare_clades_host(st_tree *tx, st_tree *ty, const int32_t *parent, int64_t n_nodes, const int64_t *ids_x,
                           const int64_t *ids_y, int64_t n_links, int64_t max_links, int64_t chunk_pairs,
                           st_pair_moments *out, int64_t *out_count, int64_t *bad_id)
try {
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    int rc = compare_trees_args(tx, ty);
    if (rc != ST_OK) return rc;
    if (n_nodes != ty->n_nodes)
        return fail(ST_ERR_ARG, "parent array of " + std::to_string(n_nodes) + " nodes: tree_y has " + std::to_string(ty->n_nodes));
    if (n_links < 0) return fail(ST_ERR_ARG, "n_links < 0");
    if (n_links > 0 && (!ids_x || !ids_y)) return fail(ST_ERR_ARG, "ids_x or ids_y is NULL");
    rc = chunk_pairs_arg(chunk_pairs);
    if (rc != ST_OK) return rc;
    rc = compare_check_ids(tx, ty, ids_x, ids_y, n_links, bad_id);
    if (rc != ST_OK) return rc;
    CladePlan P;
    std::string err;
    rc = clade_plan(parent, n_nodes, ids_y, n_links, max_links, P, err);      // (not ST_ERR_BOUNDS: ids_y were checked above)
    if (rc != ST_OK) return fail(rc, err);
    if (out_count) std::copy(P.count.begin(), P.count.end(), out_count);
    CladeTables T;
    if (!clade_tables(P, T)) return fail(ST_ERR_ARG, "more than 2^31 - 1 pieces");
    CladeReduce red{P, T, out, max_links};
    if (P.total == 0) return red.done();      // (nothing to launch)
    return clades_run(tx, ty, ids_x, ids_y, n_links, chunk_pairs > 0 ? chunk_pairs : kCladeChunkPairs, red, bad_id);
} ST_CATCH_ALL

int st_compare_rows_host(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t n_rows, int64_t m,
                         int64_t chunk_pairs, st_pair_moments *out, int64_t *bad_id)
try {
    if (n_rows < 0 || m < 0) return fail(ST_ERR_ARG, "n_rows < 0 or m < 0");
    int rc = chunk_pairs_arg(chunk_pairs);
    if (rc != ST_OK) return rc;
    if (m > 3000000000LL) return fail(ST_ERR_ARG, "m too large");
    if (n_rows > 0 && m > 0 && (!ids_x || !ids_y)) return fail(ST_ERR_ARG, "ids_x or ids_y is NULL");
    if (n_rows > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    rc = compare_trees_args(tx, ty);
    if (rc != ST_OK) return rc;
    const RowsLayout L = rows_layout(n_rows, m, chunk_pairs);
    if (L.S > 0 && n_rows > ((int64_t)1 << 50) / L.S) return fail(ST_ERR_ARG, "more than 2^50 pairs in one call");
    std::fill_n(out, n_rows, moments_empty());
    if (n_rows == 0 || L.P == 0) return ST_OK;      // (nothing to launch)
    const int64_t n_ids = n_rows * m;
    rc = compare_check_ids(tx, ty, ids_x, ids_y, n_ids, bad_id);
    if (rc != ST_OK) return rc;
    return rows_run(tx, ty, ids_x, ids_y, n_rows, m, L, out, bad_id);
} ST_CATCH_ALL

int st_quartets_host(st_tree *t, const int64_t *quartets, int64_t n, int64_t stride0, int64_t stride1,
                     int64_t *out_topologies, int64_t *bad_id)
try {
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    if (n < 0) return fail(ST_ERR_ARG, "n < 0");
    if (n > 0 && (!quartets || !out_topologies)) return fail(ST_ERR_ARG, "quartets or output is NULL");
    if (n == 0) return ST_OK;
    return quartets_host_run(t, quartets, n, stride0, stride1, out_topologies, bad_id);
} ST_CATCH_ALL

int st_quartet_positions(int device, int mode, uint64_t seed, int64_t m, int64_t k_begin, int64_t k_count, int32_t *out_pos)
try {
    std::string err;
    const int rc = quartet_range_args(mode, m, k_begin, k_count, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (k_count > 0 && !out_pos) return fail(ST_ERR_ARG, "out_pos is NULL");
    if (k_count == 0) return ST_OK;
    if (device < 0) {
        quartet_positions_host(mode, seed, m, k_begin, k_count, out_pos);
        return ST_OK;
    }
    return quartet_positions_device(device, mode, seed, m, k_begin, k_count, out_pos);
} ST_CATCH_ALL

int st_compare_quartets_leaves_host(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t m, int mode,
                                    uint64_t seed, int64_t k_begin, int64_t k_count, int64_t chunk_quartets, st_quartet_table *out,
                                    int64_t *bad_id)
try {
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    int rc = compare_trees_args(tx, ty);
    if (rc != ST_OK) return rc;
    std::string err;
    rc = quartet_range_args(mode, m, k_begin, k_count, err);
    if (rc == ST_OK) rc = quartet_chunk_arg(chunk_quartets, err);
    if (rc != ST_OK) return fail(rc, err);
    if (m > 0 && (!ids_x || !ids_y)) return fail(ST_ERR_ARG, "ids_x or ids_y is NULL");
    *out = st_quartet_table{};
    if (k_count == 0) return ST_OK;
    rc = compare_check_ids(tx, ty, ids_x, ids_y, m, bad_id);
    if (rc != ST_OK) return rc;
    return quartet_leaves_run(tx, ty, ids_x, ids_y, m, mode, seed, k_begin, k_count, chunk_quartets > 0 ? chunk_quartets : kQuartetChunk, out,
                              bad_id);
} ST_CATCH_ALL

int st_compare_quartets_host(st_tree *tx, st_tree *ty, const int64_t *quartets_x, const int64_t *quartets_y, int64_t n,
                             int64_t chunk_quartets, st_quartet_table *out, int64_t *bad_id)
try {
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    int rc = compare_trees_args(tx, ty);
    if (rc != ST_OK) return rc;
    if (n < 0) return fail(ST_ERR_ARG, "n < 0");
    std::string err;
    rc = quartet_chunk_arg(chunk_quartets, err);
    if (rc != ST_OK) return fail(rc, err);
    if (n > 0 && (!quartets_x || !quartets_y)) return fail(ST_ERR_ARG, "quartets_x or quartets_y is NULL");
    *out = st_quartet_table{};
    if (n == 0) return ST_OK;
    rc = compare_check_ids(tx, ty, quartets_x, quartets_y, 4 * n, bad_id);
    if (rc != ST_OK) return rc;
    return quartet_given_run(tx, ty, quartets_x, quartets_y, n, chunk_quartets > 0 ? chunk_quartets : kQuartetChunk, out, bad_id);
} ST_CATCH_ALL

int st_hommola_permutation(int device, uint64_t seed, int32_t node, int64_t p, int side, int32_t n, int32_t *out)
try {
    std::string err;
    const int rc = perm_args(node, p, side, n, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (!out) return fail(ST_ERR_ARG, "out is NULL");
    if (device < 0) {
        perm_host(seed, node, p, side, n, out);
        return ST_OK;
    }
    return hommola_permutation_device(device, seed, node, p, side, n, out);
} ST_CATCH_ALL

int st_hommola_clades_host(st_tree *to, st_tree *tc, const int64_t *univ_o, int32_t n_univ_o, const int64_t *univ_c, int32_t n_univ_c,
                           const int32_t *pos_o, const int32_t *pos_c, int64_t n_links, const st_hommola_clade *clades, int64_t n_clades,
                           int64_t permutations, uint64_t seed, int64_t chunk_blocks, st_pair_moments *out, int64_t *bad_id)
try {
    HommolaPlan P;
    std::string err;
    int rc = hommola_plan(n_univ_o, n_univ_c, pos_o, pos_c, n_links, clades, n_clades, permutations, chunk_blocks, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if ((n_univ_o > 0 && !univ_o) || (n_univ_c > 0 && !univ_c)) return fail(ST_ERR_ARG, "univ_o or univ_c is NULL");
    if (P.n_rows > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    rc = compare_trees_args(to, tc);
    if (rc != ST_OK) return rc;
    rc = compare_check_ids(univ_o, n_univ_o, to->n_nodes, bad_id);
    if (rc == ST_OK) rc = compare_check_ids(univ_c, n_univ_c, tc->n_nodes, bad_id);
    if (rc != ST_OK) return rc;
    std::fill_n(out, P.n_rows, moments_empty());
    if (P.n_blocks == 0) return ST_OK;      // (no clades, no links, or no clade with two links: nothing to launch)
    return hommola_clades_run(to, tc, univ_o, univ_c, pos_o, pos_c, n_links, P, seed, out, bad_id);
} ST_CATCH_ALL

// The tree side of a set entry's checks, after its plan's, in this order: univ NULL, out NULL where the call has records to
// write, the tree NULL, then the ids against the tree -- the root first, where the entry takes one
static int set_tree_args(const st_tree *t, const int64_t *univ, int32_t n_univ, bool out_missing, const int64_t *root, int64_t *bad_id)
{
    if (!univ) return fail(ST_ERR_ARG, "univ is NULL");
    if (out_missing) return fail(ST_ERR_ARG, "out is NULL");
    if (!t) return fail(ST_ERR_ARG, "tree is NULL");
    const int rc = root ? compare_check_ids(root, 1, t->n_nodes, bad_id) : ST_OK;
    return rc == ST_OK ? compare_check_ids(univ, n_univ, t->n_nodes, bad_id) : rc;
}

int st_partner_dispersion_host(st_tree *t, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                               int64_t n_sets, int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                               st_dispersion_record *out, int64_t *bad_id)
try {
    DispersionPlan P;
    std::string err;
    int rc = dispersion_plan(n_univ, set_pos, n_pos, sets, n_sets, permutations, stream, chunk_tasks, P, err);
    if (rc != ST_OK) return fail(rc, err);
    rc = set_tree_args(t, univ, n_univ, n_sets > 0 && !out, nullptr, bad_id);
    if (rc != ST_OK) return rc;
    if (P.chunks.empty()) {      // (no set of two positions: nothing to launch)
        std::fill_n(out, P.n_sets * P.rows, st_dispersion_record{0.0, 0.0});
        return ST_OK;
    }
    return record_tree_run("partner dispersion", t, univ, P, set_pos, n_pos, seed, stream, out, bad_id);
} ST_CATCH_ALL

int st_dispersion_matrix(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets,
                         int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks, st_dispersion_record *out)
try {
    DispersionPlan P;
    std::string err;
    const int rc = dispersion_plan(n, set_pos, n_pos, sets, n_sets, permutations, stream, chunk_tasks, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (!D) return fail(ST_ERR_ARG, "D is NULL");
    if (n_sets > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    if (device < 0 || P.chunks.empty()) {
        dispersion_host(D, P, set_pos, sets, seed, stream, out);
        return ST_OK;
    }
    return record_matrix_device("dispersion matrix", device, D, P, set_pos, n_pos, seed, stream, out);
} ST_CATCH_ALL

int st_swap_null_tables(int device, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t p_begin,
                        int64_t n_perms, int64_t iterations, uint64_t seed, int32_t stream, uint16_t *out, int64_t *accepted)
try {
    SwapPlan S;
    std::string err;
    const int rc = swap_tables_args(n_univ, set_pos, n_pos, sets, n_sets, p_begin, n_perms, iterations, stream, S, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (n_perms > 0 && n_pos > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    if (n_perms == 0) return ST_OK;
    if (device < 0) {
        std::vector<uint16_t> none(1);
        for (int64_t p = 0; p < n_perms; p++)
            swap_chain_host(S, set_pos, sets, seed, stream, p_begin + p, n_pos > 0 ? out + p * n_pos : none.data(), accepted ? accepted + p : nullptr);
        return ST_OK;
    }
    return swap_tables_device(device, S, set_pos, sets, p_begin, n_perms, seed, stream, out, accepted);
} ST_CATCH_ALL

int st_swap_null_schedule(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t p, int64_t iterations,
                          uint64_t seed, int32_t stream, uint16_t *out, int64_t *accepted, int64_t *steps)
try {
    SwapPlan S;
    std::string err;
    const int rc = swap_tables_args(n_univ, set_pos, n_pos, sets, n_sets, p, 1, iterations, stream, S, err);
    if (rc != ST_OK) return fail(rc, err);
    if (n_pos > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    std::vector<uint16_t> none(1);
    int64_t n_steps = 0;
    swap_chain_host(S, set_pos, sets, seed, stream, p, n_pos > 0 ? out : none.data(), accepted, true, &n_steps);
    if (steps) *steps = n_steps;
    return ST_OK;
} ST_CATCH_ALL

int st_dispersion_matrix_swap(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets,
                              int64_t permutations, int64_t iterations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                              st_dispersion_record *out, int64_t *accepted)
try {
    DispersionPlan P;
    SwapPlan S;
    std::string err;
    const int rc = swap_dispersion_plan(n, set_pos, n_pos, sets, n_sets, permutations, iterations, stream, chunk_tasks, P, S, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (!D) return fail(ST_ERR_ARG, "D is NULL");
    if (n_sets > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    if (device < 0 || P.chunks.empty()) {
        swap_dispersion_host(D, P, S, set_pos, sets, seed, stream, out, accepted);
        return ST_OK;
    }
    return swap_record_matrix_device("swap dispersion matrix", device, D, P, S, set_pos, sets, seed, stream, out, accepted);
} ST_CATCH_ALL

int st_partner_dispersion_swap_host(st_tree *t, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                                    int64_t n_sets, int64_t permutations, int64_t iterations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                                    st_dispersion_record *out, int64_t *accepted, int64_t *bad_id)
try {
    DispersionPlan P;
    SwapPlan S;
    std::string err;
    int rc = swap_dispersion_plan(n_univ, set_pos, n_pos, sets, n_sets, permutations, iterations, stream, chunk_tasks, P, S, err);
    if (rc != ST_OK) return fail(rc, err);
    rc = set_tree_args(t, univ, n_univ, n_sets > 0 && !out, nullptr, bad_id);
    if (rc != ST_OK) return rc;
    if (P.chunks.empty()) {      // (no set of two positions: no record to compute, the chains run on the host)
        std::fill_n(out, P.n_sets * P.rows, st_dispersion_record{0.0, 0.0});
        swap_accepted_host(S, set_pos, sets, P.rows, seed, stream, accepted);
        return ST_OK;
    }
    return swap_record_tree_run("partner dispersion (swap null)", t, univ, P, S, set_pos, sets, seed, stream, out, accepted, bad_id);
} ST_CATCH_ALL

int st_beta_dispersion_host(st_tree *t, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                            int64_t n_sets, int64_t begin, int64_t count, int32_t exclude_shared, int64_t permutations, uint64_t seed, int32_t stream,
                            int64_t chunk_tasks, st_dispersion_record *out, int64_t *bad_id)
try {
    SetpairPlan P;
    std::string err;
    int rc = setpair_plan(n_univ, set_pos, n_pos, sets, n_sets, begin, count, exclude_shared, permutations, stream, chunk_tasks, P, err);
    if (rc != ST_OK) return fail(rc, err);
    rc = set_tree_args(t, univ, n_univ, count > 0 && !out, nullptr, bad_id);
    if (rc != ST_OK) return rc;
    if (P.chunks.empty()) {      // (no pair, or none with two members to compare: nothing to launch)
        std::fill_n(out, 2 * P.count * P.rows, st_dispersion_record{0.0, 0.0});
        return ST_OK;
    }
    return record_tree_run("beta dispersion", t, univ, P, set_pos, n_pos, seed, stream, out, bad_id);
} ST_CATCH_ALL

int st_beta_dispersion_matrix(int device, const float *D, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets,
                              int64_t begin, int64_t count, int32_t exclude_shared, int64_t permutations, uint64_t seed, int32_t stream,
                              int64_t chunk_tasks, st_dispersion_record *out)
try {
    SetpairPlan P;
    std::string err;
    const int rc = setpair_plan(n, set_pos, n_pos, sets, n_sets, begin, count, exclude_shared, permutations, stream, chunk_tasks, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (!D) return fail(ST_ERR_ARG, "D is NULL");
    if (count > 0 && !out) return fail(ST_ERR_ARG, "out is NULL");
    if (device < 0 || P.chunks.empty()) {
        setpair_host(D, P, set_pos, n_pos, sets, seed, stream, out);
        return ST_OK;
    }
    return record_matrix_device("beta dispersion matrix", device, D, P, set_pos, n_pos, seed, stream, out);
} ST_CATCH_ALL

int st_unifrac_quantise(const float *d, const float *h, int32_t n, int32_t shift, int64_t *out_dq, int64_t *out_hq, int32_t *out_shift)
try {
    std::string err;
    const int rc = unifrac_quantise(d, h, n, shift, out_dq, out_hq, out_shift, err);
    return rc == ST_OK ? ST_OK : fail(rc, err);
} ST_CATCH_ALL

int st_unifrac_depths(int device, const int64_t *d_q, const int64_t *h_q, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                      int64_t n_sets, int64_t k_begin, int64_t k_count, int64_t chunk_pairs, int64_t *out_pd, int64_t *out_union)
try {
    UnifracPlan P;
    std::string err;
    int rc = unifrac_plan(n, set_pos, n_pos, sets, n_sets, k_begin, k_count, chunk_pairs, out_pd != nullptr, out_union != nullptr, P, err);
    if (rc == ST_OK) rc = unifrac_depth_args(d_q, h_q, n, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (P.chunks.empty()) return ST_OK;      // (no sets, an empty range or no output: nothing to launch)
    if (device < 0) {
        unifrac_host(d_q, h_q, P, set_pos, sets, out_pd, out_union);
        return ST_OK;
    }
    return unifrac_depths_device(device, P, d_q, h_q, set_pos, n_pos, sets, out_pd, out_union);
} ST_CATCH_ALL

int st_unifrac_host(st_tree *t, int64_t root, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                    int64_t n_sets, int64_t k_begin, int64_t k_count, int32_t shift, int64_t chunk_pairs, int64_t *out_pd, int64_t *out_union,
                    int32_t *out_shift, float *out_d, float *out_h, int64_t *bad_id)
try {
    UnifracPlan P;
    std::string err;
    int rc = unifrac_plan(n_univ, set_pos, n_pos, sets, n_sets, k_begin, k_count, chunk_pairs, out_pd != nullptr, out_union != nullptr, P, err);
    if (rc == ST_OK) rc = unifrac_shift_arg(shift, err);
    if (rc != ST_OK) return fail(rc, err);
    rc = set_tree_args(t, univ, n_univ, false, &root, bad_id);
    if (rc != ST_OK) return rc;
    if (n_sets == 0) {      // (no sets: nothing to launch, and no depth is asked for)
        if (out_shift) *out_shift = std::max(shift, 0);
        return ST_OK;
    }
    return unifrac_tree_run(t, root, univ, P, set_pos, n_pos, sets, shift, out_pd, out_union, out_shift, out_d, out_h, bad_id);
} ST_CATCH_ALL

int st_unifrac_null_depths(int device, const int64_t *d_q, const int64_t *h_q, int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                           int64_t n_sets, int64_t k_begin, int64_t k_count, int64_t permutations, uint64_t seed, int32_t stream, int64_t chunk_tasks,
                           int64_t *out_pd, int64_t *out_union)
try {
    UnifracNullPlan P;
    std::string err;
    int rc = unifrac_null_plan(n, set_pos, n_pos, sets, n_sets, k_begin, k_count, permutations, stream, chunk_tasks, out_pd != nullptr,
                               out_union != nullptr, P, err);
    if (rc == ST_OK) rc = unifrac_depth_args(d_q, h_q, n, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (P.chunks.empty()) return ST_OK;      // (no sets, or no output asked for: nothing to launch)
    if (device < 0) {
        unifrac_null_host(d_q, h_q, P, set_pos, n_pos, sets, seed, stream, out_pd, out_union);
        return ST_OK;
    }
    return unifrac_null_device(device, P, d_q, h_q, set_pos, n_pos, sets, seed, stream, out_pd, out_union);
} ST_CATCH_ALL

int st_unifrac_null_host(st_tree *t, int64_t root, const int64_t *univ, int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets,
                         int64_t n_sets, int64_t k_begin, int64_t k_count, int32_t shift, int64_t permutations, uint64_t seed, int32_t stream,
                         int64_t chunk_tasks, int64_t *out_pd, int64_t *out_union, int32_t *out_shift, int64_t *bad_id)
try {
    UnifracNullPlan P;
    std::string err;
    int rc = unifrac_null_plan(n_univ, set_pos, n_pos, sets, n_sets, k_begin, k_count, permutations, stream, chunk_tasks, out_pd != nullptr,
                               out_union != nullptr, P, err);
    if (rc == ST_OK) rc = unifrac_shift_arg(shift, err);
    if (rc != ST_OK) return fail(rc, err);
    rc = set_tree_args(t, univ, n_univ, false, &root, bad_id);
    if (rc != ST_OK) return rc;
    if (n_sets == 0) {      // (no sets: nothing to launch, and no depth is asked for)
        if (out_shift) *out_shift = std::max(shift, 0);
        return ST_OK;
    }
    return unifrac_null_tree_run(t, root, univ, P, set_pos, n_pos, sets, shift, seed, stream, out_pd, out_union, out_shift, bad_id);
} ST_CATCH_ALL

int st_clade_ranges(const int32_t *parent, int64_t n_nodes, const int64_t *leaf_ids, int32_t m, int32_t rooted, int32_t *out_order,
                    int32_t *out_node, int32_t *out_lo, int32_t *out_hi, int32_t *out_n, int64_t *bad_id)
try {
    if (!out_order || !out_node || !out_lo || !out_hi || !out_n) return fail(ST_ERR_ARG, "an output is NULL");
    std::vector<int32_t> order, node, lo, hi;
    std::string err;
    const int rc = clade_ranges(parent, n_nodes, leaf_ids, m, rooted != 0, order, node, lo, hi, bad_id, err);
    if (rc == ST_ERR_BOUNDS) return fail(rc, "a leaf id out of bounds (tree size: " + std::to_string(n_nodes) + ")");
    if (rc != ST_OK) return fail(rc, err);
    std::copy(order.begin(), order.end(), out_order);
    std::copy(node.begin(), node.end(), out_node);
    std::copy(lo.begin(), lo.end(), out_lo);
    std::copy(hi.begin(), hi.end(), out_hi);
    *out_n = (int32_t)node.size();
    return ST_OK;
} ST_CATCH_ALL

int st_clade_match(int device, int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo,
                   const int32_t *b_hi, int32_t n_b, int32_t unrooted, int64_t chunk_rows, int32_t *out_distance, int32_t *out_match,
                   int32_t *out_intersection)
try {
    std::string err;
    const int rc = clade_match_args(m, pos_b, a_lo, a_hi, n_a, b_lo, b_hi, n_b, chunk_rows, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (n_a > 0 && (!out_distance || !out_match || !out_intersection)) return fail(ST_ERR_ARG, "an output is NULL");
    if (n_a == 0) return ST_OK;      // (no rows: nothing to launch)
    if (device < 0) {
        clade_match_host(m, pos_b, a_lo, a_hi, n_a, b_lo, b_hi, n_b, unrooted != 0, out_distance, out_match, out_intersection);
        return ST_OK;
    }
    CladeMatchPlan P;
    clade_match_plan(m, a_lo, a_hi, n_a, b_lo, b_hi, n_b, unrooted != 0, chunk_rows, clade_match_window(), P);
    return clade_match_device(device, P, pos_b, a_lo, a_hi, out_distance, out_match, out_intersection);
} ST_CATCH_ALL

int st_mantel_codes(int device, const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, int64_t permutations, uint64_t seed, int32_t stream,
                    int64_t chunk_tasks, st_mantel_moments *moments, st_mantel_sums *out)
try {
    MantelPlan P;
    std::string err;
    const int rc = mantel_plan(x_sq, y, z, n, permutations, stream, chunk_tasks, moments, out, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0) {
        mantel_host(x_sq, y, z, P, seed, stream, out);
        return ST_OK;
    }
    return mantel_device(device, P, x_sq, y, z, seed, stream, out);
} ST_CATCH_ALL

int st_mantel_quantise(const double *v, int64_t n, int32_t shift_or_auto, int32_t *out, int32_t *out_shift)
try {
    std::string err;
    const int rc = mantel_quantise(v, n, shift_or_auto, out, out_shift, err);
    return rc == ST_OK ? ST_OK : fail(rc, err);
} ST_CATCH_ALL

int st_group_sums_codes(int device, const int32_t *y, int32_t n, const uint8_t *group, int32_t n_groups, int64_t permutations, uint64_t seed,
                        int32_t stream, int64_t chunk_tasks, int64_t *out)
try {
    GroupPlan P;
    std::string err;
    const int rc = group_plan(y, n, group, n_groups, permutations, stream, chunk_tasks, perm_slice_env("SUCHTREE_AMD_GROUP_SLICE", kGroupSlice, kGroupSliceMax), out, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0) {
        group_host(y, group, P, seed, stream, out);
        return ST_OK;
    }
    return group_device(device, P, y, group, seed, stream, out);
} ST_CATCH_ALL

int st_class_sums_codes(int device, const int32_t *y, const uint8_t *cls, int32_t n, int32_t n_classes, int64_t permutations, uint64_t seed,
                        int32_t stream, int64_t chunk_tasks, int64_t *out)
try {
    ClassPlan P;
    std::string err;
    const int rc = class_plan(y, cls, n, n_classes, permutations, stream, chunk_tasks, perm_slice_env("SUCHTREE_AMD_CLASS_SLICE", kClassSlice, kClassSliceMax), out, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0) {
        class_host(y, cls, P, seed, stream, out);
        return ST_OK;
    }
    return class_device(device, P, y, cls, seed, stream, out);
} ST_CATCH_ALL

int st_parafit_codes(int device, const int32_t *g_f, int32_t n_f, const int32_t *g_s, int32_t n_s, const int32_t *link_f, const int32_t *link_s,
                     int32_t n_links, const int32_t *stream_f, int64_t permutations, uint64_t seed, int64_t chunk_tasks, st_parafit_sum *total,
                     st_parafit_sum *link_obs, int64_t *link_n_ge, st_parafit_sum *link_all)
try {
    ParafitPlan P;
    std::string err;
    const int rc = parafit_plan(g_f, n_f, g_s, n_s, link_f, link_s, n_links, stream_f, permutations, chunk_tasks, total, link_obs, link_n_ge, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0) {
        parafit_host(g_f, g_s, P, link_f, link_s, seed, total, link_obs, link_n_ge, link_all);
        return ST_OK;
    }
    return parafit_device(device, P, g_f, g_s, link_f, link_s, seed, total, link_obs, link_n_ge, link_all);
} ST_CATCH_ALL

int st_linkage_codes(int device, const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, st_linkage_row *out_rows)
try {
    std::string err;
    const int rc = linkage_args(codes, n, weights, method, out_rows, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0) {
        linkage_host(codes, n, weights, method, out_rows);
        return ST_OK;
    }
    return linkage_device(device, codes, n, weights, method, out_rows);
} ST_CATCH_ALL

int st_rf_tasks(int device, int32_t m, int32_t n_trees, const int32_t *where, const int64_t *clade_offsets, const int32_t *lo, const int32_t *hi,
                int32_t unrooted, const int32_t *align, int32_t n_align, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p,
                int64_t n_tasks, int64_t begin, int64_t chunk_tasks, int32_t *out_shared, int64_t *out_count)
try {
    RfPlan P;
    std::string err;
    const int rc = rf_plan(m, n_trees, where, clade_offsets, lo, hi, unrooted != 0, align, n_align, task_i, task_j, task_p, n_tasks, begin, chunk_tasks,
                           out_shared, P, err);
    if (rc != ST_OK) return fail(rc, err);
    if (device_or_host_arg(device) != ST_OK) return ST_ERR_ARG;
    if (device < 0 || n_tasks == 0) {      // (no tasks: nothing to launch; the counts are zeros)
        rf_host(P, task_i, task_j, task_p, out_shared, out_count);
        return ST_OK;
    }
    return rf_device(device, P, task_i, task_j, task_p, out_shared, out_count);
} ST_CATCH_ALL

int st_graph_matrices_host(int device, int64_t n, int64_t n_edges, const int32_t *u, const int32_t *v,
                           const double *w, double *out_adjacency, double *out_laplacian)
try {
    if (n <= 0 || n_edges < 0) return fail(ST_ERR_ARG, "bad sizes");
    if (n_edges > 0 && (!u || !v || !w)) return fail(ST_ERR_ARG, "edge arrays are NULL");
    if (!out_adjacency && !out_laplacian) return fail(ST_ERR_ARG, "both outputs are NULL");
    for (int64_t e = 0; e < n_edges; e++)
        if (u[e] < 0 || u[e] >= n || v[e] < 0 || v[e] >= n) return fail(ST_ERR_ARG, "edge endpoint out of range");
    return graph_matrices_run(device, n, n_edges, u, v, w, out_adjacency, out_laplacian);
} ST_CATCH_ALL

int st_device_malloc(int device, int64_t bytes, void **out)
try {
    if (!out || bytes < 0) return fail(ST_ERR_ARG, "bad arguments");
    ST_DEVICE(device);
    ST_HIP(hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16)));
    return ST_OK;
} ST_CATCH_ALL

int st_device_free(int device, void *ptr)
try {
    ST_DEVICE(device);
    ST_HIP(hipFree(ptr));
    return ST_OK;
} ST_CATCH_ALL

int st_memcpy_h2d(int device, void *dst, const void *src, int64_t bytes)
try {
    ST_DEVICE(device);
    ST_HIP(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return ST_OK;
} ST_CATCH_ALL

int st_memcpy_d2h(int device, void *dst, const void *src, int64_t bytes)
try {
    ST_DEVICE(device);
    ST_HIP(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return ST_OK;
} ST_CATCH_ALL

int st_device_synchronize(int device)
try {
    ST_DEVICE(device);
    ST_HIP(hipDeviceSynchronize());
    return ST_OK;
} ST_CATCH_ALL

}  // extern "C"
