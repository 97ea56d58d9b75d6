// unifrac_plan.h -- the host-only side of Faith's PD and the union sums behind UniFrac (st_unifrac_host,
// st_unifrac_depths), plain C++17, and what the device shares with it (kernels_unifrac.h): the limits, the pair order,
// the range-minimum query and the lane / wave threshold.  No GPU calls in here (unifrac_plan.cpp): the "not gpu" tests
// run it under the address / undefined-behaviour sanitizers (tests/emu/sanitize_unifrac.cpp).  The definitions are the
// contract of include/suchtree_hip.h (st_unifrac_host).
//
// Layout.  A task is a pair of sets (j, i): first the n_sets tasks (r, r), whose union sum is PD(r), then the pairs
// [k_begin, k_begin + k_count) of the triangle k = i (i - 1) / 2 + j.  Either kind is cut into chunks of up to `chunk`
// tasks; a chunk holds tasks of one kind.  Every sum is an int64 over quantised depths (|q| < 2^40, at most 2^21 terms):
// exact, so nothing depends on the order of a merge, on the kernel form or on the cut.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "plan_checks.h"      // ST_QUARTET_HD, the public header, the pair order (unifrac_pair)

namespace st {

constexpr int32_t kUnifracMaxUniverse = ST_UNIFRAC_MAX_UNIVERSE;
constexpr int kUnifracLaneMax = ST_UNIFRAC_LANE_MAX;          // pairs of |A| + |B| up to this: one lane merges them; above: one wave
constexpr int kUnifracThreads = 256;                          // the workgroup of every kernel
constexpr int kUnifracWaveBlocks = 2048;                      // the fixed grid that drains a chunk's heavy pairs
constexpr int64_t kUnifracChunkPairs = (int64_t)1 << 22;      // default tasks per chunk: 32 MiB of results
constexpr int64_t kUnifracMaxChunkPairs = (int64_t)1 << 30;   // a launch's task index stays within 32 bits
constexpr int64_t kUnifracQLimit = (int64_t)1 << 40;          // |q| stays below this
constexpr int kUnifracMaxShift = 256;                         // an explicit shift: 0 .. this

// levels of the sparse table over m = n - 1 adjacent depths: l = 0 .. floor(log2 m)
ST_QUARTET_HD int unifrac_levels(int64_t m)
{
    int L = 0;
    while (m > 0) {
        L++;
        m >>= 1;
    }
    return L;
}

// min h_q[x .. y - 1], 0 <= x < y <= m, over the table M (level l at M + l * m: M[l][k] = min h_q[k .. k + 2^l - 1])
ST_QUARTET_HD int64_t unifrac_rmq(const int64_t *M, int64_t m, int32_t x, int32_t y)
{
    const int l = 31 - __builtin_clz((unsigned)(y - x));
    const int64_t *row = M + (int64_t)l * m;
    const int64_t a = row[x], b = row[y - ((int32_t)1 << l)];
    return a < b ? a : b;
}

enum UnifracKind { kUnifracPD = 0, kUnifracPairs = 1 };

struct UnifracChunk {
    int kind;                   // kUnifracPD: tasks (r, r), r from `begin`; kUnifracPairs: triangle pairs from `begin`
    int64_t begin, count;       // 1 <= count <= the plan's max_chunk
    int64_t out_at;             // where its results go: out_pd + out_at or out_union + out_at
};

struct UnifracPlan {
    int32_t n = 0;              // the universe
    int64_t m = 0;              // n - 1 adjacent depths, the row stride of the table
    int levels = 0;
    int64_t n_sets = 0, k_begin = 0, k_count = 0;
    std::vector<UnifracChunk> chunks;
    int64_t max_chunk = 0;
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: the universe size (1 .. kUnifracMaxUniverse), nothing negative
// (chunk_pairs, the range), at most 2^30 sets, the set table (position_sets_args, plan_checks.h: the counts, NULL arrays,
// set by set its offsets and its positions), the range inside the triangle of n_sets (n_sets - 1) / 2 pairs.  Then the
// layout above: PD chunks if want_pd, pair chunks if want_union; chunk_pairs 0 = kUnifracChunkPairs.
int unifrac_plan(int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count,
                 int64_t chunk_pairs, bool want_pd, bool want_union, UnifracPlan &P, std::string &err);

// ST_ERR_ARG unless shift is -1 (automatic) or 0 .. kUnifracMaxShift
int unifrac_shift_arg(int32_t shift, std::string &err);

// q(v) = llrint(ldexp((double) v, shift)) of d[0 .. n) and h[0 .. n - 1).  shift -1: 39 - ilogb(max |v|), 0 when that
// maximum is 0.  ST_ERR_ARG: n outside 1 .. kUnifracMaxUniverse, a value that is not finite, a shift outside
// -1 .. kUnifracMaxShift, a |q| of 2^40 or more.  d_q / h_q may be NULL (the checks and the shift alone).
int unifrac_quantise(const float *d, const float *h, int32_t n, int32_t shift, int64_t *d_q, int64_t *h_q, int32_t *shift_used, std::string &err);

// ST_ERR_ARG if a |d_q| or |h_q| is 2^40 or more
int unifrac_depth_args(const int64_t *d_q, const int64_t *h_q, int32_t n, std::string &err);

// the table of unifrac_rmq: levels * m entries, level 0 = h_q
void unifrac_table(const int64_t *h_q, int64_t m, int levels, int64_t *M);

// U(A, B): the reference loop, a two-pointer merge with one query per step
int64_t unifrac_union(const int64_t *d_q, const int64_t *M, int64_t m, const int32_t *A, int64_t na, const int32_t *B, int64_t nb);

// the same sum in the successor form of the wave kernel: every element of A, then those of B not in A, finds its successor
// in the union by binary search
int64_t unifrac_union_successor(const int64_t *d_q, const int64_t *M, int64_t m, const int32_t *A, int64_t na, const int32_t *B, int64_t nb);

// every task of the plan on the host, chunk by chunk; out_pd / out_union may be NULL where the plan holds no such chunk
void unifrac_host(const int64_t *d_q, const int64_t *h_q, const UnifracPlan &P, const int32_t *set_pos, const int64_t *sets, int64_t *out_pd,
                  int64_t *out_union);

}  // namespace st
