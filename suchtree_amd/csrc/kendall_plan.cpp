// kendall_plan.cpp -- see kendall_plan.h.  Integer arithmetic over caller-supplied arrays: no GPU calls.
#include "kendall_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace st {

void kendall_finish(int64_t n, int64_t n_nan, uint64_t discordant, uint64_t ties_x, uint64_t ties_y, uint64_t ties_xy,
                    st_kendall_counts *out)
{
    *out = st_kendall_counts{n, n_nan, 0, 0, 0, 0};
    if (n_nan > 0 || n == 0) return;
    out->discordant = discordant;
    out->ties_x = ties_x;
    out->ties_y = ties_y;
    out->ties_xy = ties_xy;
}

int kendall_args(const float *x, const float *y, int64_t n, const st_kendall_counts *out, std::string &err)
{
    if (!out) { err = "out is NULL"; return ST_ERR_ARG; }
    if (n < 0) { err = "n < 0"; return ST_ERR_ARG; }
    if (n > kRankMaxPairs) { err = "Kendall counts of " + std::to_string(n) + " pairs: at most " + std::to_string(kRankMaxPairs); return ST_ERR_ARG; }
    if (n > 0 && (!x || !y)) { err = "x or y is NULL"; return ST_ERR_ARG; }
    return ST_OK;
}

namespace {

// the keys of the pairs; returns the pairs that hold a NaN (their keys are not used)
int64_t kendall_keys(const float *x, const float *y, int64_t n, std::vector<uint64_t> &keys)
{
    keys.assign((size_t)n, 0);
    int64_t n_nan = 0;
    for (int64_t i = 0; i < n; i++) {
        uint32_t bx, by;
        std::memcpy(&bx, x + i, 4);
        std::memcpy(&by, y + i, 4);
        if (rank_is_nan(bx) || rank_is_nan(by)) n_nan++;
        else keys[(size_t)i] = kendall_key(bx, by);
    }
    return n_nan;
}

// sum of t (t - 1) / 2 over the runs of equal (key >> shift) of a sorted array
template <typename Key>
uint64_t tie_sum(const std::vector<Key> &sorted, int shift)
{
    uint64_t sum = 0;
    const size_t n = sorted.size();
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && (sorted[j] >> shift) == (sorted[i] >> shift)) j++;
        sum += kendall_tie_term((uint64_t)(j - i));
        i = j;
    }
    return sum;
}

// bottom-up merge sort of v with its inversion count (left first on equality)
uint64_t sort_count_inversions(std::vector<uint32_t> &v)
{
    const size_t n = v.size();
    std::vector<uint32_t> tmp(n);
    uint64_t inv = 0;
    for (size_t run = 1; run < n; run *= 2) {
        for (size_t left = 0; left < n; left += 2 * run) {
            const size_t mid = std::min(n, left + run), end = std::min(n, left + 2 * run);
            size_t i = left, j = mid, k = left;
            while (i < mid || j < end) {
                if (j >= end || (i < mid && v[i] <= v[j])) tmp[k++] = v[i++];
                else {
                    tmp[k++] = v[j++];
                    inv += (uint64_t)(mid - i);
                }
            }
        }
        v.swap(tmp);
    }
    return inv;
}

// The kernels' route over one array: tiles sorted lane by lane and level by level (k_kendall_tile_sort), then merge
// levels one output tile at a time (k_kendall_merge).  Returns the inversions when Count.
template <bool Count, typename Key>
uint64_t sort_tiled(std::vector<Key> &keys, int64_t tile)
{
    const int64_t n = (int64_t)keys.size();
    const int lanes = (int)((tile + kKendallLaneKeys - 1) / kKendallLaneKeys);
    std::vector<Key> s[2] = {std::vector<Key>((size_t)lanes * kKendallLaneKeys), std::vector<Key>((size_t)lanes * kKendallLaneKeys)};
    uint64_t inv = 0;
    for (int64_t base = 0; base < n; base += tile) {
        const int len = (int)std::min<int64_t>(tile, n - base);
        for (int lane = 0; lane < lanes; lane++) {
            Key k[kKendallLaneKeys];
            for (int j = 0; j < kKendallLaneKeys; j++) {
                const int i = lane * kKendallLaneKeys + j;
                k[j] = i < len ? keys[(size_t)(base + i)] : (Key) ~(Key)0;
            }
            inv += kendall_lane_sort<Count, Key>(k);
            for (int j = 0; j < kKendallLaneKeys; j++) s[0][(size_t)(lane * kKendallLaneKeys + j)] = k[j];
        }
        int cur = 0;
        for (int run = kKendallLaneKeys; run < len; run <<= 1, cur ^= 1)
            for (int lane = 0; lane < lanes; lane++) inv += kendall_tile_level<Count, Key>(s[cur].data(), s[cur ^ 1].data(), len, run, lane);
        std::copy(s[cur].begin(), s[cur].begin() + len, keys.begin() + base);
    }
    std::vector<Key> other((size_t)n), in((size_t)lanes * kKendallLaneKeys), out((size_t)lanes * kKendallLaneKeys);
    for (int64_t run = tile; run < n; run <<= 1) {
        const Key *src = keys.data();
        for (int64_t base = 0; base < n; base += tile) {
            const int len = (int)std::min<int64_t>(tile, n - base);
            const KendallRun R = kendall_run(base, run, n);
            const int64_t la = R.mid - R.left, lb = R.end - R.mid, d0 = base - R.left, d1 = d0 + len;
            const int64_t a0 = kendall_merge_path<int64_t, Key>(src + R.left, la, src + R.mid, lb, d0);
            const int64_t a1 = kendall_merge_path<int64_t, Key>(src + R.left, la, src + R.mid, lb, d1);
            const int na = (int)(a1 - a0), nb = len - na;
            for (int i = 0; i < len; i++) in[(size_t)i] = i < na ? src[R.left + a0 + i] : src[R.mid + (d0 - a0) + (i - na)];
            for (int lane = 0; lane < lanes; lane++)
                inv += kendall_staged_merge<Count, Key>(in.data(), na, in.data() + na, nb, lane, out.data(), (uint32_t)(la - a0));
            std::copy(out.begin(), out.begin() + len, other.begin() + base);
        }
        keys.swap(other);
    }
    return inv;
}

}  // namespace

int kendall_host(const float *x, const float *y, int64_t n, st_kendall_counts *out, std::string &err)
{
    const int rc = kendall_args(x, y, n, out, err);
    if (rc != ST_OK) return rc;
    std::vector<uint64_t> keys;
    const int64_t n_nan = kendall_keys(x, y, n, keys);
    if (n_nan > 0 || n == 0) {
        kendall_finish(n, n_nan, 0, 0, 0, 0, out);
        return ST_OK;
    }
    std::sort(keys.begin(), keys.end());
    const uint64_t ties_x = tie_sum(keys, 32), ties_xy = tie_sum(keys, 0);
    std::vector<uint32_t> low((size_t)n);
    for (int64_t i = 0; i < n; i++) low[(size_t)i] = (uint32_t)keys[(size_t)i];
    const uint64_t discordant = sort_count_inversions(low);
    kendall_finish(n, 0, discordant, ties_x, tie_sum(low, 0), ties_xy, out);
    return ST_OK;
}

int kendall_host_tiled(const float *x, const float *y, int64_t n, int64_t tile, st_kendall_counts *out, std::string &err)
{
    const int rc = kendall_args(x, y, n, out, err);
    if (rc != ST_OK) return rc;
    if (tile < 1 || tile > ((int64_t)1 << 24)) { err = "tile out of range"; return ST_ERR_ARG; }
    std::vector<uint64_t> keys;
    const int64_t n_nan = kendall_keys(x, y, n, keys);
    if (n_nan > 0 || n == 0) {
        kendall_finish(n, n_nan, 0, 0, 0, 0, out);
        return ST_OK;
    }
    (void)sort_tiled<false, uint64_t>(keys, tile);
    const uint64_t ties_x = tie_sum(keys, 32), ties_xy = tie_sum(keys, 0);
    std::vector<uint32_t> low((size_t)n);
    for (int64_t i = 0; i < n; i++) low[(size_t)i] = (uint32_t)keys[(size_t)i];
    const uint64_t discordant = sort_tiled<true, uint32_t>(low, tile);
    kendall_finish(n, 0, discordant, ties_x, tie_sum(low, 0), ties_xy, out);
    return ST_OK;
}

}  // namespace st
