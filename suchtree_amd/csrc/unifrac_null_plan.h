// unifrac_null_plan.h -- the host-only side of Faith's PD and the union sums under the taxa-labels null
// (st_unifrac_null_host, st_unifrac_null_depths), plain C++17.  No GPU calls in here (unifrac_null_plan.cpp): the "not gpu"
// tests run it under the address / undefined-behaviour sanitizers (tests/emu/sanitize_unifrac_null.cpp).  The definitions
// are the contract of include/suchtree_hip.h (st_unifrac_null_host); the depths, the table and U(A, B) are those of
// unifrac_plan.h, the permutation blocks and the chunks those of dispersion_plan.h.
//
// Layout.  An item is a set r (items 0 .. n_sets) or, where union sums are asked for, a pair of the range (item n_sets +
// k - k_begin).  Within a block of n_perms permutations from p0, task t = item * n_perms + (p - p0) is that item under
// permutation p, as in DispersionPlan: the set tasks of a block come first, and they leave the block's relabelled table
// (n_perms x n_pos positions of 16 bits: row p - p0 is set_pos relabelled, every set's R_p in ascending order at the
// set's own offsets) for its pair tasks.  A chunk is a range of t of one block and may hold tasks of both kinds.  Where
// only union sums are asked for the set tasks still run, to write the table; their sums are dropped.
// (The pair kernels take a chunk's pair tasks as rectangles of pairs x rows, the pair fastest: host_unifrac_null.h.)
#pragma once
#include "dispersion_plan.h"
#include "unifrac_plan.h"

namespace st {

struct UnifracNullPlan {
    int32_t n = 0;              // the universe
    int64_t m = 0;              // n - 1 adjacent depths, the row stride of the table
    int levels = 0;
    int64_t n_sets = 0, k_begin = 0, k_count = 0, rows = 0;      // rows = permutations + 1 values per set and per pair
    bool want_pd = false, want_union = false;
    int64_t items = 0;          // n_sets, plus k_count where union sums are asked for; 0: nothing to do
    int64_t n_tab = 0;          // entries of a row of the relabelled table: n_pos, or 0 where no union sum is asked for
    int64_t perm_block = 0;
    std::vector<DispersionChunk> chunks;
    int64_t max_chunk_tasks = 0;
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: those of dispersion_call_args (the universe size, nothing
// negative among permutations, chunk_tasks and stream), the set table (position_sets_args, plan_checks.h), then the
// range: nothing negative, at most 2^30 sets, inside the triangle of n_sets (n_sets - 1) / 2 pairs, at most 2^40 values
// per output array.  Then the layout above, cut by dispersion_cut with the table's n_tab entries a permutation
// counted beside the sigma row.
int unifrac_null_plan(int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count,
                      int64_t permutations, int32_t stream, int64_t chunk_tasks, bool want_pd, bool want_union, UnifracNullPlan &P,
                      std::string &err);

// every value of the call on the host: for each p, sigma by perm_host, every set relabelled and sorted, unifrac_union
void unifrac_null_host(const int64_t *d_q, const int64_t *h_q, const UnifracNullPlan &P, const int32_t *set_pos, int64_t n_pos,
                       const int64_t *sets, uint64_t seed, int32_t stream, int64_t *out_pd, int64_t *out_union);

// results[n] of tasks [task_begin, task_begin + n) of the block at p_begin into out_pd / out_union (a NULL one is skipped)
void unifrac_null_scatter(const UnifracNullPlan &P, const DispersionChunk &c, const int64_t *results, int64_t *out_pd, int64_t *out_union);

}  // namespace st
