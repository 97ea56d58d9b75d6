// dispersion_plan.h -- the host-only side of the partner-dispersion reduction (st_partner_dispersion_host,
// st_dispersion_matrix), plain C++17, and what the device shares with it (kernels_dispersion.h): the size classes and the
// record.  No GPU calls in here (dispersion_plan.cpp): the "not gpu" tests run it under the address /
// undefined-behaviour sanitizers (tests/emu/sanitize_dispersion.cpp).  The definitions are the contract of
// include/suchtree_hip.h (st_partner_dispersion_host).
//
// Layout.  A task is (set, permutation p).  Sets of fewer than two positions make no task: their records are zeros.
// The others are ordered by size class -- K' = 2, 4, 8, 16, 32 (packed: 64 / K' tasks per wave), 64 (one task per wave),
// then the sets of more than 64 positions (one task per workgroup) -- and by their index within a class.  The
// permutations are cut into blocks of up to `perm_block` consecutive p, whose sigma rows the device holds at once; within
// a block of n_perms permutations from p0, task t = c * n_perms + (p - p0) is set order[c] under permutation p, so a
// class is one range of t, and a chunk is a range of t of one block.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "keyed_perm.h"

namespace st {

constexpr int kDispersionWaveMax = 64;            // sets of up to 64 positions: element i in lane i
constexpr int kDispersionPackedMax = 32;          // K' up to 32: several tasks per wave
constexpr int kDispersionThreads = 256;           // the workgroup of every task kernel
constexpr int kDispersionClasses = 7;             // K' = 2 .. 64 (classes 0 .. 5), then the workgroup class (6)
constexpr int64_t kDispersionChunkTasks = 1 << 20;            // default tasks per chunk: 16 MiB of records
constexpr int64_t kDispersionMaxChunkTasks = 1 << 30;          // a launch's task index stays within 32 bits
constexpr int64_t kDispersionSigmaBytes = 64 << 20;           // default bound of a block's sigma rows

// K' of a set of k >= 2 positions, k <= 64: max(2, the next power of two >= k)
ST_QUARTET_HD int dispersion_lanes(int k)
{
    int kp = 2;
    while (kp < k) kp <<= 1;
    return kp;
}
ST_QUARTET_HD int dispersion_class(int k)      // k >= 2
{
    if (k > kDispersionWaveMax) return 6;
    int c = 0;
    for (int kp = 2; kp < k; kp <<= 1) c++;
    return c;
}

struct DispersionSetDev {
    int begin, count;      // the set's positions: set_pos[begin, begin + count)
};

struct DispersionChunk {
    int64_t p_begin, n_perms;          // the block of permutations it belongs to
    int64_t task_begin, n_tasks;       // tasks [task_begin, task_begin + n_tasks) of that block
};

struct DispersionPlan {
    int32_t n_univ = 0;
    int64_t n_sets = 0, rows = 0;                 // rows = permutations + 1 records per set
    std::vector<int64_t> order;                   // the live sets (k >= 2) by (class, index)
    std::vector<DispersionSetDev> sets;           // order[c]'s range
    int64_t class_begin[kDispersionClasses + 1] = {};      // sets [class_begin[k], class_begin[k + 1]) of `order` are of class k
    int64_t perm_block = 0;
    int max_count = 0;                            // the largest set
    std::vector<DispersionChunk> chunks;
    int64_t max_chunk_tasks = 0;
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: the universe size (3 .. kPermMaxUniverse), nothing negative
// (permutations, chunk_tasks, stream), at most 2^40 records, then the set table (position_sets_args, plan_checks.h: the
// counts, NULL arrays, set by set its offsets and its positions).  Then the layout above: chunk_tasks 0 = blocks of up
// to kDispersionSigmaBytes of sigma rows and chunks of kDispersionChunkTasks tasks; chunk_tasks > 0 = at most that many
// tasks per chunk and permutations per block.
int dispersion_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t permutations,
                    int32_t stream, int64_t chunk_tasks, DispersionPlan &P, std::string &err);

// What the other plan units share with this one.  The first checks of a call, in this order: the universe size, nothing
// negative (permutations, chunk_tasks, stream).  What a wave does with `a += shfl_xor(a, o)` over offsets width / 2 .. 1:
// v[0 .. width) in, every lane's total out.
int dispersion_call_args(int32_t n_univ, int64_t permutations, int64_t chunk_tasks, int32_t stream, std::string &err);

// permutations per task `slice` >= 1: the slices of n_perms permutations, the last one shorter (group_plan.h, class_plan.h)
inline int64_t dispersion_slices(int64_t n_perms, int32_t slice) { return (n_perms + slice - 1) / slice; }

// The one cut of `rows` permutations into blocks and chunks, by the rule above.  A block is up to `block` permutations (the
// caller's bound, whatever holds a block's rows; below 1 counts as 1) and has live * dispersion_slices(its permutations,
// slice) tasks: `live` tasks a permutation where slice = 1.  chunk_tasks 0 = chunks of kDispersionChunkTasks tasks;
// chunk_tasks > 0 = at most that many tasks per chunk and permutations per block.  live = 0: no chunk.
void dispersion_cut_blocks(int64_t rows, int64_t live, int64_t block, int64_t chunk_tasks, int64_t &perm_block, std::vector<DispersionChunk> &chunks,
                           int64_t &max_chunk_tasks, int32_t slice = 1);
// the cut of the set plans: blocks of up to kDispersionSigmaBytes of sigma rows; a caller that keeps `table_entries` further
// 16-bit entries a permutation beside the sigma row (unifrac_null_plan.cpp) has them counted towards the block's bound
void dispersion_cut(int32_t n_univ, int64_t rows, int64_t live, int64_t chunk_tasks, int64_t &perm_block, std::vector<DispersionChunk> &chunks,
                    int64_t &max_chunk_tasks, int64_t table_entries = 0);

// What the matrix permutation plans have in common (MantelPlan, GroupPlan, ClassPlan, ParafitPlan): a statistic of whole
// matrices under every permutation, one item (the wave form) or `items` rows of work a permutation, folded block by block
// on the device (matrix_block_chunks, host_dispersion.h).
struct MatrixPlan {
    int64_t rows = 0;             // permutations + 1 records
    bool wave = false;
    int64_t items = 0;            // 1 (wave form), or the row form's items a permutation
    int64_t perm_block = 0;
    std::vector<DispersionChunk> chunks;
    int64_t max_chunk_tasks = 0;
};
// its cut: dispersion_cut_blocks over its rows and items
inline void matrix_cut(MatrixPlan &P, int64_t block, int64_t chunk_tasks, int32_t slice = 1)
{
    dispersion_cut_blocks(P.rows, P.items, block, chunk_tasks, P.perm_block, P.chunks, P.max_chunk_tasks, slice);
}

// A matrix plan whose row form gives a task `slice` permutations of one row pair (GroupPlan, ClassPlan).  n > 64: an item is
// a row pair r < (n + 1) / 2 -- rows r and n - 1 - r, the middle row alone when n is odd; a block of n_perms permutations
// from p0 is cut into n_slices = dispersion_slices(n_perms, slice) and task t = r * n_slices + s is row pair r under slice
// s.  Up to 64: the wave form, one item, task t is permutation p0 + t of the block.
struct SlicedPlan : MatrixPlan {
    int32_t n = 0;
    int32_t slice = 0;            // permutations per task of the row form
};
// the tasks of a block of n_perms permutations
inline int64_t sliced_block_tasks(const SlicedPlan &P, int64_t n_perms) { return P.items * dispersion_slices(n_perms, P.wave ? 1 : P.slice); }
inline size_t sliced_stride(int32_t n) { return ((size_t)n + 15) & ~(size_t)15; }      // bytes of a row of n bytes that 16-byte loads read

// The first checks of the matrix plans over one universe (mantel, group, class): those of dispersion_call_args, then at
// most 2^31 - 1 permutations.
int matrix_call_args(int32_t n, int64_t permutations, int64_t chunk_tasks, int32_t stream, std::string &err);
// ST_OK, or ST_ERR_ARG naming the first cell (row-major) of the n x n matrix x, called `name`, whose mirror differs
int symmetric_arg(const char *name, const int32_t *x, int32_t n, std::string &err);
void dispersion_butterfly(double *v, int width);

// `order` by (size class, `before` within a class, index) and the class ranges of the layout above: cls(x) is the size
// class of item x, before(a, b) a tie-break within a class (none: the items of a class stay in the order they came in)
template <typename Cls, typename Before>
void dispersion_order(std::vector<int64_t> &order, int64_t (&class_begin)[kDispersionClasses + 1], Cls cls, Before before)
{
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const int ca = cls(a), cb = cls(b);
        return ca != cb ? ca < cb : before(a, b);
    });
    const int64_t live = (int64_t)order.size();
    int64_t c = 0;
    for (int k = 0; k < kDispersionClasses; k++) {
        class_begin[k] = c;
        while (c < live && cls(order[(size_t)c]) == k) c++;
    }
    class_begin[kDispersionClasses] = live;
}

// The lane-order tail of a record over k elements, by the order rule of the contract: element(i, sum, near) gives element
// i's two terms.  Up to 64 elements, element i sits in lane i of K' lanes and one butterfly adds them; above, lane i % 256
// adds its elements in ascending order from 0.0, every wave runs its butterfly and the wave totals are added in wave order.
template <typename Element>
st_dispersion_record dispersion_lane_order(int32_t k, Element element)
{
    const bool wave = k <= kDispersionWaveMax;
    const int lanes = wave ? dispersion_lanes(k) : kDispersionThreads;
    double a[kDispersionThreads], b[kDispersionThreads];
    std::fill(a, a + lanes, 0.0);
    std::fill(b, b + lanes, 0.0);
    for (int32_t i = 0; i < k; i++) {
        double sum, near;
        element(i, sum, near);
        if (wave) {
            a[i] = sum;
            b[i] = near;
        } else {
            a[i % kDispersionThreads] += sum;
            b[i % kDispersionThreads] += near;
        }
    }
    for (int w = 0; w < lanes; w += 64) {
        dispersion_butterfly(a + w, std::min(lanes, 64));
        dispersion_butterfly(b + w, std::min(lanes, 64));
    }
    st_dispersion_record out{a[0], b[0]};
    for (int w = 64; w < lanes; w += 64) {
        out.pair_sum += a[w];
        out.nearest_sum += b[w];
    }
    return out;
}

// the record of the relabelled positions q[0 .. k) over the n x n matrix D, by the order rule of the contract
st_dispersion_record dispersion_record(const float *D, int32_t n, const int32_t *q, int32_t k);

// every record of the call on the host: out[r * rows + p]
void dispersion_host(const float *D, const DispersionPlan &P, const int32_t *set_pos, const int64_t *sets, uint64_t seed, int32_t stream,
                     st_dispersion_record *out);

// entry j of chunk c: task t = c.task_begin + j is item `item` of the plan's order under permutation p
inline void dispersion_task_of(const DispersionChunk &c, int64_t j, int64_t &item, int64_t &p)
{
    const int64_t t = c.task_begin + j;
    item = t / c.n_perms;
    p = c.p_begin + t % c.n_perms;
}

// records[n] of tasks [task_begin, task_begin + n) of the block at p_begin into out, for a plan of records (DispersionPlan,
// SetpairPlan: item s of the order is row order[s] of out)
template <typename Plan>
void dispersion_scatter(const Plan &P, const DispersionChunk &c, const st_dispersion_record *records, st_dispersion_record *out)
{
    for (int64_t j = 0; j < c.n_tasks; j++) {
        int64_t s, p;
        dispersion_task_of(c, j, s, p);
        out[P.order[(size_t)s] * P.rows + p] = records[j];
    }
}

}  // namespace st
