// kendall_plan.h -- the host-only side of exact Kendall's tau-b (st_compare_*_kendall_host, st_kendall_arrays_host,
// st_kendall_host), plain C++17, and the inline functions the device shares with it (kernels_kendall.h): the 64-bit
// key of a pair, the bounds of the runs a merge level joins, the merge-path search, a lane's serial merge with its
// inversion count and tie rule, a lane's sort of its own keys.  No GPU calls in here (kendall_plan.cpp): the "not gpu"
// tests run it under the address / undefined-behaviour sanitizers.
//
// Definition (include/suchtree_hip.h: st_kendall_counts).  Over the n pairs of a call, n0 = n (n - 1) / 2,
// ties_x = sum over x's tie groups of t (t - 1) / 2, ties_y likewise, ties_xy over groups equal in both,
// discordant = #{i, j} with (x_i - x_j)(y_i - y_j) < 0.  Sort the pairs by (x, y): the discordant pairs are then the
// inversions of the y sequence (inside an x tie group the y's ascend, so a tie never counts).  With n <= 2^31 - 1 every
// count is below 2^61: all of it is integer arithmetic, exact in any order.
//
// The sort is a merge sort in three layers that all go through kendall_lane_merge: a lane sorts its own
// kKendallLaneKeys keys (odd-even transposition: adjacent swaps, one inversion each), the lanes of a workgroup merge runs
// of 8, 16, ... keys inside a tile of ST_KENDALL_TILE keys, and merge levels join runs of tile << level keys, one
// workgroup per output tile.  A run's length is a multiple of the tile (of the lane's keys inside a tile), so an output
// tile (a lane's outputs) lies inside one pair of runs: kendall_run gives its bounds, clipped to n -- a last left run may
// be short and its right run absent (then the merge is a copy).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "rank_plan.h"

namespace st {

constexpr int kKendallLaneKeys = 8;      // keys a lane sorts by itself and merges per level
static_assert(ST_KENDALL_TILE % kKendallLaneKeys == 0, "a tile is whole lanes");
static_assert((kKendallLaneKeys & (kKendallLaneKeys - 1)) == 0, "runs inside a tile are powers of two");

// (x, y) -> the key whose unsigned order is the order by x, then y.  Not for NaN (rank_is_nan first).
ST_RANK_HD uint64_t kendall_key(uint32_t bits_x, uint32_t bits_y) { return ((uint64_t)rank_key(bits_x) << 32) | rank_key(bits_y); }

// The pair of runs of `run` keys that holds position `pos` of n keys: the left run is [left, mid), the right [mid, end).
struct KendallRun {
    int64_t left, mid, end;
};
ST_RANK_HD KendallRun kendall_run(int64_t pos, int64_t run, int64_t n)
{
    const int64_t left = pos / (2 * run) * (2 * run);
    const int64_t mid = left + run < n ? left + run : n;
    const int64_t end = left + 2 * run < n ? left + 2 * run : n;
    return KendallRun{left, mid, end};
}

// Merge path: of the first d keys of the merge of a[0, la) and b[0, lb), how many come from a.  On equality the key of a
// goes first (a holds the left run: a tie is never an inversion).
template <typename I, typename Key>
ST_RANK_HD I kendall_merge_path(const Key *a, I la, const Key *b, I lb, I d)
{
    I lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const I mid = lo + (hi - lo) / 2;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One lane's share of a merge: outputs [d, d + count) of the merge of a[0, la) and b[0, lb) go to out[0, count).  Returns
// the inversions its keys of b close: a key of b taken while r keys of the whole left run are still to come adds r;
// `left_total` is what remains of the left run at a[0] (la, or more when a is a staged piece of it).
template <bool Count, typename I, typename Key>
ST_RANK_HD uint64_t kendall_lane_merge(const Key *a, I la, const Key *b, I lb, I d, I count, Key *out, I left_total)
{
    I ia = kendall_merge_path<I, Key>(a, la, b, lb, d), ib = d - ia;
    I rem = left_total - ia;
    uint64_t inv = 0;
    for (I k = 0; k < count; k++) {
        if (ib >= lb || (ia < la && a[ia] <= b[ib])) {
            out[k] = a[ia++];
            rem--;
        } else {
            out[k] = b[ib++];
            if (Count) inv += (uint64_t)rem;
        }
    }
    return inv;
}

// A lane's outputs of one level inside a tile of `len` keys: positions [kKendallLaneKeys lane, + kKendallLaneKeys) of dst.
template <bool Count, typename Key>
ST_RANK_HD uint64_t kendall_tile_level(const Key *src, Key *dst, int len, int run, int lane)
{
    const int pos = lane * kKendallLaneKeys;
    if (pos >= len) return 0;
    // kendall_run(pos, run, len) in 32 bits without a division: run is kKendallLaneKeys << level, a power of two
    const int left = pos & ~(2 * run - 1);
    const int mid = left + run < len ? left + run : len, end = left + 2 * run < len ? left + 2 * run : len;
    const int count = end - pos < kKendallLaneKeys ? end - pos : kKendallLaneKeys;
    return kendall_lane_merge<Count, int, Key>(src + left, mid - left, src + mid, end - mid, pos - left, count, dst + pos, mid - left);
}

// A lane's outputs of a merge level from the staged pieces a[0, na) of the left run and b[0, nb) of the right run.
template <bool Count, typename Key>
ST_RANK_HD uint64_t kendall_staged_merge(const Key *a, int na, const Key *b, int nb, int lane, Key *out, uint32_t left_total)
{
    const int pos = lane * kKendallLaneKeys, total = na + nb;
    if (pos >= total) return 0;
    const int count = total - pos < kKendallLaneKeys ? total - pos : kKendallLaneKeys;
    // (left_total < 2^31: the counts of a lane stay in 32 bits, their sum is 64-bit)
    return kendall_lane_merge<Count, int, Key>(a, na, b, nb, pos, count, out + pos, (int)left_total);
}

// A lane's own keys, sorted by odd-even transposition (fixed indices: they stay in registers); pad the keys beyond the
// tile's length with the largest key, which no swap moves.  Returns the swaps = the inversions among them.
template <bool Count, typename Key>
ST_RANK_HD uint32_t kendall_lane_sort(Key (&k)[kKendallLaneKeys])
{
    uint32_t swaps = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int round = 0; round < kKendallLaneKeys; round++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = round & 1; i + 1 < kKendallLaneKeys; i += 2) {
            const Key lo = k[i], hi = k[i + 1];
            const bool swap = lo > hi;
            k[i] = swap ? hi : lo;
            k[i + 1] = swap ? lo : hi;
            if (Count) swaps += swap;
        }
    }
    return swaps;
}

// sum over the tie groups of t (t - 1) / 2, from the groups' sizes one at a time
ST_RANK_HD uint64_t kendall_tie_term(uint64_t t) { return t * (t - 1) / 2; }

// the record from the counts; n_nan > 0: every count is 0
void kendall_finish(int64_t n, int64_t n_nan, uint64_t discordant, uint64_t ties_x, uint64_t ties_y, uint64_t ties_xy,
                    st_kendall_counts *out);
// the argument checks st_kendall_host and st_kendall_arrays_host share
int kendall_args(const float *x, const float *y, int64_t n, const st_kendall_counts *out, std::string &err);

// st_kendall_host: sort the keys, tie sums from runs of the sorted keys, merge sort of the low words with an inversion
// count, ties_y from the sorted low words.
int kendall_host(const float *x, const float *y, int64_t n, st_kendall_counts *out, std::string &err);
// The same counts by the kernels' own route -- tiles of `tile` keys sorted lane by lane and level by level, then merge
// levels one output tile at a time, both sorts (64-bit keys without counting, low words with), all through the shared
// functions above -- at any tile >= 1: it pins the partition arithmetic before anything runs on a GPU.
int kendall_host_tiled(const float *x, const float *y, int64_t n, int64_t tile, st_kendall_counts *out, std::string &err);

}  // namespace st
