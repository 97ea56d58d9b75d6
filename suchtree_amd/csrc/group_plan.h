// group_plan.h -- the host-only side of the within-group sums of a distance matrix under relabelling (st_group_sums_codes:
// compare.permanova, compare.anosim), plain C++17.  No GPU calls in here (group_plan.cpp): the "not gpu" tests run it
// under the address / undefined-behaviour sanitizers (tests/emu/sanitize_group.cpp).  The definitions are the contract of
// include/suchtree_hip.h (st_group_sums_codes); the permutation, its blocks and the chunk record are those of
// dispersion_plan.h.
//
// Layout.  n > kGroupWaveMax: the row form.  An item is a row pair r < (n + 1) / 2 -- rows r and n - 1 - r, the middle
// row alone when n is odd -- so that every item has about n pairs.  A block of n_perms permutations from p0 is cut into
// n_slices = ceil(n_perms / slice) slices of `slice` permutations (the last one shorter); task t = r * n_slices + s is row
// pair r under slice s, whose workgroup stages its rows of y once for all the slice's permutations.  Up to kGroupWaveMax:
// the wave form, one item, task t is permutation p0 + t of the block.  A chunk is a range of t of one block.
#pragma once
#include "dispersion_plan.h"
#include "plan_checks.h"

namespace st {

constexpr int kGroupMax = ST_GROUP_MAX;                  // labels are bytes
constexpr int kGroupWaveMax = 64;                         // matrices of up to 64 rows: row l in lane l, y in LDS (why)
constexpr int kGroupWaveStride = kGroupWaveMax + 1;       // the wave form's LDS row stride in words: odd, so the 64 rows of a column lie in 64 banks
constexpr int kGroupThreads = 256;                        // the workgroup of every kernel
constexpr int kGroupSlice = 64;                           // permutations per task of the row form: DESIGN.md section 24 has the sweep
constexpr int kGroupSliceMax = 256;                       // bound of SUCHTREE_AMD_GROUP_SLICE
constexpr int64_t kGroupBlockItems = (int64_t)1 << 22;    // bound of a block's row pairs x permutations (two 16-byte partial records each)

struct GroupPart {      // the partial record of (row i, permutation p): the sum over j < i with G_p[j] == g
    int64_t sum;
    int32_t g;          // G_p[i]
    int32_t reserved;
};

struct GroupPlan : SlicedPlan {      // rows of out; a row of relabelled labels is sliced_stride(n) bytes
    int32_t n_groups = 0;
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: those of dispersion_call_args (n in 3 .. kPermMaxUniverse,
// nothing negative among permutations, chunk_tasks, stream), at most 2^31 - 1 permutations, n_groups in 1 .. kGroupMax,
// NULL pointers (y, group, out), then the first group[i] >= n_groups.  Then the layout above for `slice` in
// 1 .. kGroupSliceMax: chunk_tasks 0 = blocks of up to kDispersionSigmaBytes of sigma rows and kGroupBlockItems row pairs
// x permutations, chunks of kDispersionChunkTasks tasks; chunk_tasks > 0 = at most that many tasks per chunk and
// permutations per block.
int group_plan(const int32_t *y, int32_t n, const uint8_t *group, int32_t n_groups, int64_t permutations, int32_t stream, int64_t chunk_tasks,
               int32_t slice, const int64_t *out, GroupPlan &P, std::string &err);

// what row i adds under the relabelled labels G[0 .. n): the record (sum over j < i with G[j] == G[i] of y_row[j], G[i])
GroupPart group_row(const int32_t *y_row, const uint8_t *G, int32_t i);

// every row of the call on the host: out[p * n_groups + h], the relabel, the row records and the fold of the kernels
void group_host(const int32_t *y, const uint8_t *group, const GroupPlan &P, uint64_t seed, int32_t stream, int64_t *out);

}  // namespace st
