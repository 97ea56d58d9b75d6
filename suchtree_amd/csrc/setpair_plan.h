// setpair_plan.h -- the host-only side of the between-set dispersion reduction (st_beta_dispersion_host,
// st_beta_dispersion_matrix), plain C++17, and what the device shares with it (kernels_setpair.h): the task table.  No GPU
// calls in here (setpair_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour sanitizers
// (tests/emu/sanitize_setpair.cpp).  The definitions are the contract of include/suchtree_hip.h (st_beta_dispersion_host);
// the size classes, the permutation blocks, the chunks and the record are those of dispersion_plan.h.
//
// Layout.  A direction u = (k - begin) * 2 + dir of the range is a pair of sets (r -> c): lane set r, walked set c.  A
// direction with an empty r or an empty c makes no task: its records are zeros.  The others are ordered by the size class
// of k_r -- K' = 2 .. 32 (packed), 64 (one wave), then k_r > 64 (one workgroup) -- within a class by k_c, so that the
// packed tasks of a wave walk similar lengths, then by u.  Within a block of n_perms permutations from p0, task
// t = c * n_perms + (p - p0) is direction order[c] under permutation p, as in DispersionPlan.
#pragma once
#include "dispersion_plan.h"
#include "plan_checks.h"      // the pair order (unifrac_pair)

namespace st {

constexpr int64_t kSetpairMaxPairs = (int64_t)1 << 31;      // pairs per call

struct SetpairTaskDev {
    int r_begin, r_count;      // the lane set's positions: set_pos[r_begin, r_begin + r_count)
    int c_begin, c_count;      // the walked set's
};

struct SetpairPlan {
    int32_t n_univ = 0;
    int64_t n_sets = 0, rows = 0;                 // rows = permutations + 1 records per direction
    int64_t begin = 0, count = 0;                 // the range of the triangle
    int exclude = 0;
    std::vector<int64_t> order;                   // the live directions by (class of k_r, k_c, u)
    std::vector<SetpairTaskDev> tasks;            // order[c]'s two sets
    int64_t class_begin[kDispersionClasses + 1] = {};
    int64_t perm_block = 0;
    int max_walk = 0;                             // the largest walked set of a workgroup task
    std::vector<DispersionChunk> chunks;
    int64_t max_chunk_tasks = 0;
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: those of dispersion_plan -- the universe size, nothing negative
// (permutations, chunk_tasks, stream), the set table (position_sets_args, plan_checks.h) -- then the range: nothing
// negative, inside the triangle of n_sets (n_sets - 1) / 2 pairs, at most 2^31 pairs, at most 2^40 records.  Then the
// layout above, cut by dispersion_cut.
int setpair_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t begin, int64_t count,
                 int32_t exclude_shared, int64_t permutations, int32_t stream, int64_t chunk_tasks, SetpairPlan &P, std::string &err);

// the record of one direction: the lane set's relabelled positions qr[0 .. kr) and unpermuted positions sr[0 .. kr), the
// walked set's qc / sc[0 .. kc), over the n x n matrix D, by the order rule of the contract
st_dispersion_record setpair_record(const float *D, int32_t n, const int32_t *qr, const int32_t *sr, int32_t kr, const int32_t *qc,
                                    const int32_t *sc, int32_t kc, bool exclude);

// every record of the call on the host: out[u * rows + p]
void setpair_host(const float *D, const SetpairPlan &P, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, uint64_t seed, int32_t stream,
                  st_dispersion_record *out);

}  // namespace st
