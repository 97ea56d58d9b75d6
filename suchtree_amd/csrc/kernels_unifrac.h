// kernels_unifrac.h -- included by suchtree_hip.hip (after kernels_dispersion.h).
// The device side of st_unifrac_host and st_unifrac_depths (layout, pair order and the query: unifrac_plan.h; the
// contract: include/suchtree_hip.h).  Task (j, i) sums, over the distinct merged positions s_1 < ... < s_t of sets j and i,
// q(d[s_k]) minus the minimum of q(h) between s_k and its successor.  Everything is int64: no float arithmetic in here, so
// the two forms below, any grid and any chunk cut give the same integers.
//
//   k_unifrac_table   one level of the sparse table per launch: M[l][k] = min(M[l-1][k], M[l-1][k + 2^(l-1)]).
//   k_unifrac_widen   the int32 MRCA ids of adjacent universe leaves as the int64 id list of the distance kernels.
//   k_unifrac_lane    one task per lane.  The lanes of a wave share row i and walk j (the wave's first task is unranked
//                     once, with integers; a lane steps from it), so set i's positions are a broadcast and the sets j lie
//                     behind one another.  A lane merges the two lists with two pointers: one gather of d_q and one query
//                     (two gathers of the table) per merged position, each an L2 or Infinity Cache hit.  A task of more
//                     than lane_max positions is not merged here: the lane appends its index to the chunk's
//                     heavy list (a vector atomic add on a counter in global memory, zeroed per chunk).
//   k_unifrac_wave    a fixed grid drains the heavy list, whose length it reads on the device: one task per wave.  The
//                     lanes stride over the elements of A, then over those of B not in A; each finds its successor in the
//                     union by a binary search in the other list and adds q(d[x]) - min q(h[x .. next - 1]), or q(d[x])
//                     for the union's last element.  An int64 butterfly finishes the task and lane 0 stores it.
// Every result cell is written once: by its lane, or by the wave that drew it from the list.  The merge and the successor
// sum are unifrac_merge and unifrac_successor below, shared with the null's pair kernels (kernels_unifrac_null.h).
#pragma once

#include "unifrac_plan.h"

namespace st {

__global__ __launch_bounds__(kUnifracThreads) void k_unifrac_table(const int64_t *below, int64_t *row, long long half, long long count)
{
    const long long k = (long long)blockIdx.x * kUnifracThreads + threadIdx.x;
    if (k >= count) return;
    const int64_t a = below[k], b = below[k + half];
    row[k] = a < b ? a : b;
}

__global__ __launch_bounds__(kUnifracThreads) void k_unifrac_widen(const int *ids, long long *out, long long count)
{
    const long long k = (long long)blockIdx.x * kUnifracThreads + threadIdx.x;
    if (k < count) out[k] = ids[k];
}

struct UnifracArgs {
    const int64_t *d_q;          // n depths
    const int64_t *table;        // levels x m, level 0 = h_q
    const int *set_pos;
    const int64_t *sets;         // n_sets + 1 offsets
    int64_t *out;                // this chunk's results: entry t
    unsigned *heavy;             // this chunk's heavy list: up to `count` task indices ...
    unsigned *n_heavy;           // ... and its length
    long long m;                 // the table's row stride, n - 1
    long long begin;             // the chunk's first task: set r (PD) or triangle pair k
    unsigned count;              // tasks of the chunk
    int kind;                    // kUnifracPD / kUnifracPairs
    int lane_max;                // tasks of more positions go to the heavy list (kUnifracLaneMax)
};

// the sets (j, i) of task t of the chunk, from the task of lane 0 of the wave (t0: i0, j0), `step` tasks on
__device__ __forceinline__ void unifrac_step(long long &i, long long &j, unsigned step)
{
    j += step;
    while (j >= i) {      // (rows of 64 or more pairs: at most one turn)
        j -= i;
        i++;
    }
}

// U(A, B) by one lane: the two-pointer merge over the ascending lists A = pos[pa .. ea) and B = pos[pb .. eb), one gather of
// d_q and one query per merged position.  Pos is int (the caller's positions) or unsigned short (a row of the relabelled
// table of kernels_unifrac_null.h, laid out as the caller's positions are).
template <typename Pos>
__device__ __forceinline__ int64_t unifrac_merge(const int64_t *d_q, const int64_t *table, long long m, const Pos *pos, long long pa, long long ea,
                                                 long long pb, long long eb)
{
    const int none = 0x7FFFFFFF;
    int x = pa < ea ? (int)pos[pa] : none, y = pb < eb ? (int)pos[pb] : none, prev = -1;
    int64_t sum = 0;
    while (pa < ea || pb < eb) {
        const int c = x < y ? x : y;
        if (x == c) {
            pa++;
            x = pa < ea ? (int)pos[pa] : none;
        }
        if (y == c) {
            pb++;
            y = pb < eb ? (int)pos[pb] : none;
        }
        sum += d_q[c];
        if (prev >= 0) sum -= unifrac_rmq(table, m, prev, c);
        prev = c;
    }
    return sum;
}

// the first index in [lo, hi) whose position is > x (Upper) or >= x (!Upper)
template <bool Upper, typename Pos>
__device__ __forceinline__ long long unifrac_bound(const Pos *pos, long long lo, long long hi, int x)
{
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const int v = (int)pos[mid];
        if (Upper ? v <= x : v < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a lane's share of U(A, B) by one wave, the successor form, A = pos[a0 .. a1) and B = pos[b0 .. b1): the lanes stride over
// the elements of A, then over those of B not in A (none where `same`: B is A); the caller adds the 64 shares up
template <typename Pos>
__device__ __forceinline__ int64_t unifrac_successor(const int64_t *d_q, const int64_t *table, long long m, const Pos *pos, long long a0, long long a1,
                                                     long long b0, long long b1, bool same, unsigned lane)
{
    const int none = 0x7FFFFFFF;
    int64_t sum = 0;
    for (long long e = a0 + lane; e < a1; e += 64) {
        const int x = (int)pos[e], in_a = e + 1 < a1 ? (int)pos[e + 1] : none;
        const long long up = unifrac_bound<true>(pos, b0, b1, x);
        const int in_b = up < b1 ? (int)pos[up] : none, next = in_a < in_b ? in_a : in_b;
        sum += d_q[x];
        if (next != none) sum -= unifrac_rmq(table, m, x, next);
    }
    for (long long e = b0 + lane; e < b1 && !same; e += 64) {      // (a PD task: B is A, every element is counted)
        const int y = (int)pos[e], in_b = e + 1 < b1 ? (int)pos[e + 1] : none;
        const long long lo = unifrac_bound<false>(pos, a0, a1, y);
        const int in_a = lo < a1 ? (int)pos[lo] : none;
        if (in_a == y) continue;      // (counted with A)
        const int next = in_a < in_b ? in_a : in_b;
        sum += d_q[y];
        if (next != none) sum -= unifrac_rmq(table, m, y, next);
    }
    return sum;
}

__global__ __launch_bounds__(kUnifracThreads) void k_unifrac_lane(UnifracArgs a)
{
    const unsigned t = blockIdx.x * kUnifracThreads + threadIdx.x, lane = threadIdx.x & 63, t0 = t - lane;
    if (t0 >= a.count) return;      // (wave-uniform)
    long long i, j;
    if (a.kind == kUnifracPD) {
        i = j = a.begin + (t < a.count ? t : t0);
    } else {
        int64_t i0, j0;
        unifrac_pair((int64_t)(a.begin + __builtin_amdgcn_readfirstlane((int)t0)), i0, j0);
        i = i0;
        j = j0;
        unifrac_step(i, j, t < a.count ? lane : 0);
    }
    if (t >= a.count) return;
    const long long pa = a.sets[j], pb = a.sets[i], ea = a.sets[j + 1], eb = a.sets[i + 1];
    if ((ea - pa) + (eb - pb) > a.lane_max) {
        a.heavy[atomicAdd(a.n_heavy, 1u)] = t;
        return;
    }
    a.out[t] = unifrac_merge(a.d_q, a.table, a.m, a.set_pos, pa, ea, pb, eb);
}

__global__ __launch_bounds__(kUnifracThreads) void k_unifrac_wave(UnifracArgs a)
{
    const unsigned lane = threadIdx.x & 63, waves = gridDim.x * (kUnifracThreads / 64);
    const unsigned n_heavy = *a.n_heavy;      // (written by the launch before this one)
    for (unsigned w = blockIdx.x * (kUnifracThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); w < n_heavy; w += waves) {
        const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)a.heavy[w]);
        long long i, j;
        if (a.kind == kUnifracPD) {
            i = j = a.begin + t;
        } else {
            int64_t i0, j0;
            unifrac_pair((int64_t)(a.begin + t), i0, j0);
            i = i0;
            j = j0;
        }
        int64_t sum = unifrac_successor(a.d_q, a.table, a.m, a.set_pos, a.sets[j], a.sets[j + 1], a.sets[i], a.sets[i + 1], i == j, lane);
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) a.out[t] = sum;
    }
}

}  // namespace st
