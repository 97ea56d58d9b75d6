// kernels_kendall.h -- included by suchtree_hip.hip (after kernels_ranks.h).
// Exact Kendall tau-b counts of the compare path (st_compare_*_kendall_host, st_kendall_arrays_host; the definition and
// the merge arithmetic the host shares: kendall_plan.h).  The distance kernels write a chunk of float32 x[k], y[k] as
// for k_pair_moments; here every pair is kept, as one 64-bit key, and sorted:
//   k_kendall_keys               key(x) << 32 | key(y) of a chunk at the chunk's offset, and how many pairs hold a NaN
//   k_kendall_tile_sort<K, C>    tiles of ST_KENDALL_TILE keys sorted in LDS: a lane sorts its 8 keys in registers, then
//                                the lanes merge runs of 8, 16, ... keys between two LDS buffers
//   k_kendall_merge<K, C>        one level: runs of `run` keys joined in pairs, one workgroup per output tile -- two
//                                merge-path searches in global memory, the two input pieces staged in LDS, a lane's 8
//                                outputs merged serially from its own diagonal, the tile written back whole
//   k_kendall_low_words          the sorted keys' low words (y) into the spare buffer
//   k_kendall_tie_blocks / k_kendall_tie_carry / k_kendall_tie_sums
//                                sum over i of (i - start of i's run of equal key >> shift) over a sorted array: the last
//                                run start of every block, its running maximum over the blocks, then the sums
//   k_kendall_final              the per-workgroup slots of the four counts, added
// With C (Count) a sort adds the inversions it removes to its workgroup's slot: taking a right-run key while r keys
// of the left run are still to come adds r (left first on equality: a tie is no inversion).  Order of work (host_compare.h:
// KendallState::enqueue): keys, sort as uint64 without counting, tie sums of x (shift 32) and of (x, y) (shift 0), low
// words, sort as uint32 with counting = discordant, tie sum of y.  Everything is integer arithmetic: exact whatever the
// grid.  No kernel reads or writes past n; only LDS and registers are padded.
#pragma once

#include "kendall_plan.h"

namespace st {

constexpr int kKendallThreads = 256;
constexpr int kKendallBlocks = 2048;      // workgroups of every kernel (fewer when there are fewer tiles) = result slots per count
constexpr int kKendallTile = ST_KENDALL_TILE;
static_assert(kKendallTile == kKendallThreads * kKendallLaneKeys, "a lane holds kKendallLaneKeys keys of its workgroup's tile");

// slots of the four counts in the part array, kKendallBlocks each
enum { kKendallDiscordant = 0, kKendallTiesX = 1, kKendallTiesXY = 2, kKendallTiesY = 3, kKendallCounts = 4 };

// the workgroup's sum, added to its own slot (the kernels of a call run one after another on one stream)
__device__ __forceinline__ void kendall_add_to_slot(unsigned long long v, unsigned long long *__restrict__ part)
{
    __shared__ unsigned long long w_sum[kKendallThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) w_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = part[blockIdx.x];
        for (int w = 0; w < kKendallThreads / 64; w++) t += w_sum[w];
        part[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kKendallThreads) void k_kendall_keys(const float *__restrict__ x, const float *__restrict__ y, long long n,
                                                                   unsigned long long *__restrict__ keys, unsigned long long *__restrict__ n_nan)
{
    const long long lanes = (long long)gridDim.x * kKendallThreads;
    unsigned nan = 0;
    for (long long i = (long long)blockIdx.x * kKendallThreads + threadIdx.x; i < n; i += lanes) {
        const uint32_t bx = __float_as_uint(x[i]), by = __float_as_uint(y[i]);
        nan += rank_is_nan(bx) || rank_is_nan(by);
        keys[i] = kendall_key(bx, by);      // (with a NaN in the call the keys are sorted but no count is reported)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nan += __shfl_xor(nan, off);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(n_nan, (unsigned long long)nan);
}

// src == dst is allowed: a tile is read whole before it is written
template <typename Key, bool Count>
__global__ __launch_bounds__(kKendallThreads) void k_kendall_tile_sort(const Key *src, Key *dst, long long n, unsigned long long *__restrict__ part)
{
    __shared__ Key s[2][kKendallTile];
    const int tid = threadIdx.x;
    const long long n_tiles = (n + kKendallTile - 1) / kKendallTile;
    unsigned long long inv = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long base = tile * kKendallTile;
        const int len = (int)(n - base < kKendallTile ? n - base : kKendallTile);
        for (int i = tid; i < len; i += kKendallThreads) s[0][i] = src[base + i];
        __syncthreads();
        Key k[kKendallLaneKeys];
#pragma unroll
        for (int j = 0; j < kKendallLaneKeys; j++) {
            const int i = tid * kKendallLaneKeys + j;
            k[j] = i < len ? s[0][i] : (Key) ~(Key)0;
        }
        inv += kendall_lane_sort<Count, Key>(k);
#pragma unroll
        for (int j = 0; j < kKendallLaneKeys; j++) s[0][tid * kKendallLaneKeys + j] = k[j];
        __syncthreads();
        int cur = 0;
        for (int run = kKendallLaneKeys; run < len; run <<= 1) {
            inv += kendall_tile_level<Count, Key>(s[cur], s[cur ^ 1], len, run, tid);
            __syncthreads();
            cur ^= 1;
        }
        for (int i = tid; i < len; i += kKendallThreads) dst[base + i] = s[cur][i];
        __syncthreads();
    }
    if (Count) kendall_add_to_slot(inv, part);
}

template <typename Key, bool Count>
__global__ __launch_bounds__(kKendallThreads) void k_kendall_merge(const Key *__restrict__ src, Key *__restrict__ dst, long long n, long long run,
                                                                    unsigned long long *__restrict__ part)
{
    __shared__ Key s_in[kKendallTile], s_out[kKendallTile];
    __shared__ long long s_split[2];
    const int tid = threadIdx.x;
    const long long n_tiles = (n + kKendallTile - 1) / kKendallTile;
    unsigned long long inv = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long base = tile * kKendallTile;
        const int len = (int)(n - base < kKendallTile ? n - base : kKendallTile);
        const KendallRun R = kendall_run(base, run, n);
        const long long la = R.mid - R.left, lb = R.end - R.mid, d0 = base - R.left;
        if (tid < 2) s_split[tid] = kendall_merge_path<long long, Key>(src + R.left, la, src + R.mid, lb, tid ? d0 + len : d0);
        __syncthreads();
        const long long a0 = s_split[0], b0 = d0 - a0;
        const int na = (int)(s_split[1] - a0), nb = len - na;
        for (int i = tid; i < len; i += kKendallThreads) s_in[i] = i < na ? src[R.left + a0 + i] : src[R.mid + b0 + (i - na)];
        __syncthreads();
        inv += kendall_staged_merge<Count, Key>(s_in, na, s_in + na, nb, tid, s_out, (uint32_t)(la - a0));
        __syncthreads();
        for (int i = tid; i < len; i += kKendallThreads) dst[base + i] = s_out[i];
    }
    if (Count) kendall_add_to_slot(inv, part);
}

__global__ __launch_bounds__(kKendallThreads) void k_kendall_low_words(const unsigned long long *__restrict__ keys, long long n, uint32_t *__restrict__ low)
{
    const long long lanes = (long long)gridDim.x * kKendallThreads;
    for (long long i = (long long)blockIdx.x * kKendallThreads + threadIdx.x; i < n; i += lanes) low[i] = (uint32_t)keys[i];
}

// A block of the tie scan = a tile.  The lane's view of it: is key i the start of a run of equal (key >> shift)?
// s[0] holds the key before the block (any value for the first block: key 0 is a start), s[1 + i] key base + i.
template <typename Key>
__device__ __forceinline__ void kendall_tie_stage(Key *s, const Key *__restrict__ keys, long long base, int len)
{
    for (int i = threadIdx.x; i < len; i += kKendallThreads) s[1 + i] = keys[base + i];
    if (threadIdx.x == 0) s[0] = base > 0 ? keys[base - 1] : (Key)0;
    __syncthreads();
}
template <typename Key>
__device__ __forceinline__ bool kendall_tie_start(const Key *s, long long base, int i, int shift)
{
    return (base == 0 && i == 0) || (s[1 + i] >> shift) != (s[i] >> shift);
}

// step 1: last_start[b] = the index of the last run start in block b, -1 when the block has none
template <typename Key>
__global__ __launch_bounds__(kKendallThreads) void k_kendall_tie_blocks(const Key *__restrict__ keys, long long n, int shift, int *__restrict__ last_start)
{
    __shared__ Key s[kKendallTile + 1];
    __shared__ int w_max[kKendallThreads / 64];
    const long long n_blocks = (n + kKendallTile - 1) / kKendallTile;
    for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const long long base = b * kKendallTile;
        const int len = (int)(n - base < kKendallTile ? n - base : kKendallTile);
        kendall_tie_stage(s, keys, base, len);
        int m = -1;
        for (int j = 0; j < kKendallLaneKeys; j++) {
            const int i = threadIdx.x * kKendallLaneKeys + j;
            if (i < len && kendall_tie_start(s, base, i, shift)) m = (int)(base + i);      // (indices stay below 2^31)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
        if ((threadIdx.x & 63) == 0) w_max[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kKendallThreads / 64; w++) m = max(m, w_max[w]);
            last_start[b] = m;
        }
        __syncthreads();
    }
}

// step 2 (one workgroup): last_start becomes its exclusive running maximum, the start of the run that enters each block
__global__ __launch_bounds__(kKendallThreads) void k_kendall_tie_carry(int *__restrict__ last_start, long long n_blocks)
{
    __shared__ int t_max[kKendallThreads];
    const long long per = (n_blocks + kKendallThreads - 1) / kKendallThreads;
    const long long lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks;
    const long long hi = lo + per < n_blocks ? lo + per : n_blocks;
    int m = -1;
    for (long long i = lo; i < hi; i++) m = max(m, last_start[i]);
    t_max[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = -1;
        for (int i = 0; i < kKendallThreads; i++) {
            const int v = t_max[i];
            t_max[i] = run;
            run = max(run, v);
        }
    }
    __syncthreads();
    int run = t_max[threadIdx.x];
    for (long long i = lo; i < hi; i++) {
        const int v = last_start[i];
        last_start[i] = run;
        run = max(run, v);
    }
}

// step 3: sum over i of (i - start of i's run), added to the workgroup's slot
template <typename Key>
__global__ __launch_bounds__(kKendallThreads) void k_kendall_tie_sums(const Key *__restrict__ keys, long long n, int shift, const int *__restrict__ carry,
                                                                       unsigned long long *__restrict__ part)
{
    __shared__ Key s[kKendallTile + 1];
    __shared__ int w_max[kKendallThreads / 64];
    const long long n_blocks = (n + kKendallTile - 1) / kKendallTile;
    unsigned long long sum = 0;
    for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const long long base = b * kKendallTile;
        const int len = (int)(n - base < kKendallTile ? n - base : kKendallTile);
        kendall_tie_stage(s, keys, base, len);
        int m = -1;      // the last start among the lane's own keys
        for (int j = 0; j < kKendallLaneKeys; j++) {
            const int i = threadIdx.x * kKendallLaneKeys + j;
            if (i < len && kendall_tie_start(s, base, i, shift)) m = (int)(base + i);
        }
        int incl = m;      // inclusive running maximum over the wave's lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if ((int)(threadIdx.x & 63) >= off) incl = max(incl, up);
        }
        if ((threadIdx.x & 63) == 63) w_max[threadIdx.x >> 6] = incl;
        int before = __shfl_up(incl, 1);      // ... and over the lanes before this one
        if ((threadIdx.x & 63) == 0) before = -1;
        __syncthreads();
        int cur = max(carry[b], before);
        for (int w = 0; w < (int)(threadIdx.x >> 6); w++) cur = max(cur, w_max[w]);
        for (int j = 0; j < kKendallLaneKeys; j++) {
            const int i = threadIdx.x * kKendallLaneKeys + j;
            if (i < len) {
                if (kendall_tie_start(s, base, i, shift)) cur = (int)(base + i);
                sum += (unsigned long long)(base + i - cur);
            }
        }
        __syncthreads();
    }
    kendall_add_to_slot(sum, part);
}

// workgroup c (one wave) adds the slots of count c
__global__ __launch_bounds__(64) void k_kendall_final(const unsigned long long *__restrict__ part, unsigned long long *__restrict__ out)
{
    unsigned long long t = 0;
    for (int i = threadIdx.x; i < kKendallBlocks; i += 64) t += part[blockIdx.x * kKendallBlocks + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

}  // namespace st
