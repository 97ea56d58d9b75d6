// rank_plan.h -- the host-only side of exact Spearman rank correlation (st_compare_*_ranks_host, st_spearman_host),
// plain C++17, and the few inline functions the device shares with it (kernels_ranks.h): the order-preserving key of a
// float32, the layout of the sparse count tables, the midrank and tie arithmetic.  No GPU calls in here
// (rank_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour sanitizers.
//
// Definition (include/suchtree_hip.h: st_rank_sums).  For the n pairs of a call, a_k = 2 rank_x(x_k) - (n + 1) with
// rank_x the midrank, = 2 (#values < x_k) + (#values == x_k) - n, an integer; b_k likewise for y.  Sxy = sum a_k b_k,
// Sxx = sum a_k^2 = (n^3 - n - sum over x's tie groups of (t^3 - t)) / 3, Syy likewise.  With n <= 2^31 - 1,
// |a| < 2^31, |a b| < 2^62 and every sum fits 128 bits: all of it is integer arithmetic, exact in any order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/suchtree_hip.h"

#if defined(__HIP__)      // (spelled as attributes: hipcc compiles rank_plan.cpp as HIP too, without the runtime header)
#define ST_RANK_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define ST_RANK_HD inline
#endif

namespace st {

using i128 = __int128;
using u128 = unsigned __int128;

constexpr int64_t kRankMaxPairs = INT32_MAX;       // |a| stays within int32, a * b within int64
constexpr int kRankTopBits = 12, kRankLowBits = 32 - kRankTopBits;
constexpr int kRankBuckets = 1 << kRankTopBits;    // top buckets of the key space
constexpr int64_t kRankBucketKeys = (int64_t)1 << kRankLowBits;      // counters per occupied bucket (4 MiB of uint32)

ST_RANK_HD bool rank_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
// float32 bits -> uint32 whose unsigned order is the values' order: -0.0 becomes +0.0, then non-negative values get
// their sign bit set and negative ones all bits flipped.  Not for NaN (rank_is_nan first).
ST_RANK_HD uint32_t rank_key(uint32_t bits)
{
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
// a = 2 rank - (n + 1) of a value with `less` values below it and `count` equal to it (itself included)
ST_RANK_HD int32_t rank_centered(int64_t less, int64_t count, int64_t n) { return (int32_t)(2 * less + count - n); }
// t^3 - t of a tie group of t values
ST_RANK_HD u128 rank_tie_term(uint64_t t) { return (u128)t * t * t - t; }

// Occupied top buckets in key order: slot[b] = index of bucket b's 2^20 counters in the table, -1 where no value fell.
struct RankSlots {
    int32_t slot[kRankBuckets];
    int32_t n_slots = 0;
};
void rank_slots(const uint32_t *occupancy, RankSlots &S);
ST_RANK_HD int64_t rank_table_index(int32_t slot, uint32_t key)
{
    return ((int64_t)slot << kRankLowBits) | (int64_t)(key & (uint32_t)(kRankBucketKeys - 1));
}

// The record from what the passes leave: Sxy and the two tie sums.  n_nan > 0: every sum and distinct count is 0.
void rank_finish(int64_t n, int64_t n_nan, int64_t distinct_x, int64_t distinct_y, i128 sxy, u128 tie_x, u128 tie_y,
                 st_rank_sums *out);

// st_spearman_host: the same keys, midranks and tie arithmetic over two plain arrays.  (The counts live in a sorted
// array of the distinct keys here, not in 2^20 counters per occupied bucket: host arrays of arbitrary floats occupy
// hundreds of buckets, gigabytes of counters for a few thousand values.)
int spearman_host(const float *x, const float *y, int64_t n, st_rank_sums *out, std::string &err);

}  // namespace st
