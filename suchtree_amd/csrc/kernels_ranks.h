// kernels_ranks.h -- included by suchtree_hip.hip (after kernels_compare.h).
// Exact Spearman rank sums of the compare path (st_compare_*_ranks_host; the definition: rank_plan.h).  The distance
// kernels write a chunk of float32 x[k], y[k] as for k_pair_moments; these kernels never keep a pair:
//   pass 0  k_rank_occupancy   which of the 4096 top-12-bit buckets of the order-preserving key each tree's values fall
//                              in (LDS histograms, flushed with integer atomics) and how many pairs hold a NaN
//   pass 1  k_rank_count       one uint32 counter per (occupied bucket, low 20 bits): integer atomic adds, no return
//           k_rank_block_sums / k_rank_scan_blocks / k_rank_scan_apply
//                              one scan in key order: count -> a = 2 less + count - n (int32, in place), and on the
//                              way the tie sum (t^3 - t, 128 bits) and the number of distinct values
//   pass 2  k_rank_dot         a_x[x_k] * a_y[y_k] summed in 128 bits per lane, lanes and waves folded with shuffles
//                              into the workgroup's own slot; k_rank_dot_final adds the slots
// Everything is integer arithmetic: the result is exact whatever the order of the atomics, the grid or the chunks.
// A value whose bucket pass 0 did not see (it cannot happen: every pass recomputes the same distances) is skipped and
// counted in `miss`, which fails the call; no index leaves its table.
#pragma once

#include "rank_plan.h"

namespace st {

constexpr int kRankBlocks = 1024;        // workgroups of the per-pair kernels and of k_rank_block_sums
constexpr int kRankThreads = 256;
constexpr int kRankScanBlock = 4096;     // counters per scan block: 16 per lane
static_assert(kRankBucketKeys % kRankScanBlock == 0, "a bucket is whole scan blocks");

// what pass 0 leaves: occupancy of tree X's buckets, then tree Y's, then the NaN pairs
struct RankOccupancy {
    unsigned occ[2 * kRankBuckets];
    unsigned long long n_nan;
};
// one workgroup's (and the final) share of a scan: the tie sum, the distinct values, the values counted
struct RankScanPart {
    unsigned long long tie_lo, tie_hi, distinct, total;
};
struct RankDotPart {
    unsigned long long lo;
    long long hi;
};

__device__ __forceinline__ u128 rank_u128(unsigned long long lo, unsigned long long hi) { return ((u128)hi << 64) | lo; }

// the pairs of a chunk as k_pair_moments takes them: quads q = lane, lane + lanes, ..., then the n % 4 tail
template <typename F>
__device__ __forceinline__ void rank_for_pairs(const float *__restrict__ x, const float *__restrict__ y, long long n, F f)
{
    const long long lanes = (long long)gridDim.x * kRankThreads;
    const long long lane = (long long)blockIdx.x * kRankThreads + threadIdx.x;
    const long long quads = n >> 2;
    const uint4 *x4 = reinterpret_cast<const uint4 *>(x);
    const uint4 *y4 = reinterpret_cast<const uint4 *>(y);
    for (long long q = lane; q < quads; q += lanes) {
        const uint4 a = x4[q], b = y4[q];
        f(a.x, b.x);
        f(a.y, b.y);
        f(a.z, b.z);
        f(a.w, b.w);
    }
    if (lane < (n & 3)) {
        const long long i = (quads << 2) + lane;
        f(__float_as_uint(x[i]), __float_as_uint(y[i]));
    }
}

__global__ __launch_bounds__(kRankThreads) void k_rank_occupancy(const float *__restrict__ x, const float *__restrict__ y, long long n,
                                                                  RankOccupancy *__restrict__ out)
{
    __shared__ unsigned h[2 * kRankBuckets];
    for (int i = threadIdx.x; i < 2 * kRankBuckets; i += kRankThreads) h[i] = 0u;
    __syncthreads();
    unsigned nan = 0;
    rank_for_pairs(x, y, n, [&](uint32_t bx, uint32_t by) {
        if (rank_is_nan(bx) || rank_is_nan(by)) {
            nan++;
            return;
        }
        atomicAdd(&h[rank_key(bx) >> kRankLowBits], 1u);
        atomicAdd(&h[kRankBuckets + (rank_key(by) >> kRankLowBits)], 1u);
    });
    __syncthreads();
    // (a workgroup sees at most 2^25 / kRankBlocks pairs per chunk, a call at most 2^31 - 1: no counter overflows)
    for (int i = threadIdx.x; i < 2 * kRankBuckets; i += kRankThreads) {
        const unsigned v = h[i];
        if (v) atomicAdd(&out->occ[i], v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nan += __shfl_xor(nan, off);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&out->n_nan, (unsigned long long)nan);
}

// slots: tree X's 4096 bucket -> slot entries, then tree Y's (-1: not occupied)
__device__ __forceinline__ void rank_load_slots(int *s, const int *__restrict__ slots)
{
    for (int i = threadIdx.x; i < 2 * kRankBuckets; i += kRankThreads) s[i] = slots[i];
    __syncthreads();
}

__global__ __launch_bounds__(kRankThreads) void k_rank_count(const float *__restrict__ x, const float *__restrict__ y, long long n,
                                                              const int *__restrict__ slots, unsigned *__restrict__ tab_x,
                                                              unsigned *__restrict__ tab_y, unsigned *__restrict__ miss)
{
    __shared__ int s[2 * kRankBuckets];
    rank_load_slots(s, slots);
    unsigned missed = 0;
    rank_for_pairs(x, y, n, [&](uint32_t bx, uint32_t by) {
        const uint32_t kx = rank_key(bx), ky = rank_key(by);
        const int sx = s[kx >> kRankLowBits], sy = s[kRankBuckets + (ky >> kRankLowBits)];
        if (rank_is_nan(bx) || rank_is_nan(by) || sx < 0 || sy < 0) {
            missed++;
            return;
        }
        (void)__hip_atomic_fetch_add(tab_x + rank_table_index(sx, kx), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(tab_y + rank_table_index(sy, ky), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    if (missed) atomicAdd(miss, missed);
}

// Scan, step 1: block_sum[b] = the values counted in scan block b (lane t holds counters [16 t, 16 t + 16) of it);
// workgroup w takes blocks w, w + grid, ... and leaves its share of the tie sum and the distinct count in part[w].
__global__ __launch_bounds__(kRankThreads) void k_rank_block_sums(const unsigned *__restrict__ tab, long long n_blocks,
                                                                   unsigned long long *__restrict__ block_sum,
                                                                   RankScanPart *__restrict__ part)
{
    __shared__ unsigned long long w_sum[kRankThreads / 64];
    __shared__ RankScanPart w_part[kRankThreads / 64];
    u128 tie = 0;
    unsigned long long distinct = 0;
    for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint4 *p = reinterpret_cast<const uint4 *>(tab + b * kRankScanBlock) + threadIdx.x * 4;
        unsigned long long sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint4 v = p[j];
            const unsigned c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sum += c[k];
                distinct += c[k] != 0u;
                if (c[k] > 1u) tie += rank_tie_term(c[k]);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if ((threadIdx.x & 63) == 0) w_sum[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int w = 0; w < kRankThreads / 64; w++) t += w_sum[w];
            block_sum[b] = t;
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        tie += rank_u128(__shfl_xor((unsigned long long)tie, off), __shfl_xor((unsigned long long)(tie >> 64), off));
        distinct += __shfl_xor(distinct, off);
    }
    if ((threadIdx.x & 63) == 0) w_part[threadIdx.x >> 6] = RankScanPart{(unsigned long long)tie, (unsigned long long)(tie >> 64), distinct, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        u128 t = 0;
        unsigned long long d = 0;
        for (int w = 0; w < kRankThreads / 64; w++) {
            t += rank_u128(w_part[w].tie_lo, w_part[w].tie_hi);
            d += w_part[w].distinct;
        }
        part[blockIdx.x] = RankScanPart{(unsigned long long)t, (unsigned long long)(t >> 64), d, 0};
    }
}

// Scan, step 2 (one workgroup): block_sum becomes its exclusive prefix; the n_parts shares are added into *out, whose
// `total` is the number of values counted.
__global__ __launch_bounds__(kRankThreads) void k_rank_scan_blocks(unsigned long long *__restrict__ block_sum, long long n_blocks,
                                                                    const RankScanPart *__restrict__ part, int n_parts,
                                                                    RankScanPart *__restrict__ out)
{
    __shared__ unsigned long long t_sum[kRankThreads + 1];
    __shared__ RankScanPart t_part[kRankThreads];
    const long long per = (n_blocks + kRankThreads - 1) / kRankThreads;
    const long long lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks;
    const long long hi = lo + per < n_blocks ? lo + per : n_blocks;
    unsigned long long sum = 0;
    for (long long i = lo; i < hi; i++) sum += block_sum[i];
    t_sum[threadIdx.x] = sum;
    u128 tie = 0;
    unsigned long long distinct = 0;
    for (int i = threadIdx.x; i < n_parts; i += kRankThreads) {
        tie += rank_u128(part[i].tie_lo, part[i].tie_hi);
        distinct += part[i].distinct;
    }
    t_part[threadIdx.x] = RankScanPart{(unsigned long long)tie, (unsigned long long)(tie >> 64), distinct, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        u128 t = 0;
        unsigned long long d = 0;
        for (int i = 0; i < kRankThreads; i++) {
            const unsigned long long v = t_sum[i];
            t_sum[i] = run;
            run += v;
            t += rank_u128(t_part[i].tie_lo, t_part[i].tie_hi);
            d += t_part[i].distinct;
        }
        *out = RankScanPart{(unsigned long long)t, (unsigned long long)(t >> 64), d, run};
    }
    __syncthreads();
    unsigned long long run = t_sum[threadIdx.x];
    for (long long i = lo; i < hi; i++) {
        const unsigned long long v = block_sum[i];
        block_sum[i] = run;
        run += v;
    }
}

// Scan, step 3: one workgroup per scan block; every counter becomes a = 2 less + count - n (int32 in the same four
// bytes; the a of an empty counter is never read).
__global__ __launch_bounds__(kRankThreads) void k_rank_scan_apply(unsigned *__restrict__ tab, const unsigned long long *__restrict__ block_off,
                                                                   long long n)
{
    __shared__ unsigned w_sum[kRankThreads / 64];
    uint4 *p = reinterpret_cast<uint4 *>(tab + (long long)blockIdx.x * kRankScanBlock) + threadIdx.x * 4;
    uint4 v[4];
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = p[j];
        sum += v[j].x + v[j].y + v[j].z + v[j].w;
    }
    unsigned incl = sum;      // (a block's values are at most n < 2^31)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off);
        if ((int)(threadIdx.x & 63) >= off) incl += up;
    }
    if ((threadIdx.x & 63) == 63) w_sum[threadIdx.x >> 6] = incl;
    __syncthreads();
    long long less = (long long)block_off[blockIdx.x] + (incl - sum);
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) less += w_sum[w];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        unsigned c[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned count = c[k];
            c[k] = (unsigned)rank_centered(less, count, n);
            less += count;
        }
        p[j] = make_uint4(c[0], c[1], c[2], c[3]);
    }
}

// `first` (the call's first chunk) writes the workgroup's slot instead of adding to it
__global__ __launch_bounds__(kRankThreads) void k_rank_dot(const float *__restrict__ x, const float *__restrict__ y, long long n,
                                                            const int *__restrict__ slots, const int *__restrict__ a_x,
                                                            const int *__restrict__ a_y, int first, RankDotPart *__restrict__ part,
                                                            unsigned *__restrict__ miss)
{
    __shared__ int s[2 * kRankBuckets];
    __shared__ RankDotPart w_part[kRankThreads / 64];
    rank_load_slots(s, slots);
    unsigned missed = 0;
    i128 acc = 0;
    rank_for_pairs(x, y, n, [&](uint32_t bx, uint32_t by) {
        const uint32_t kx = rank_key(bx), ky = rank_key(by);
        const int sx = s[kx >> kRankLowBits], sy = s[kRankBuckets + (ky >> kRankLowBits)];
        if (rank_is_nan(bx) || rank_is_nan(by) || sx < 0 || sy < 0) {
            missed++;
            return;
        }
        acc += (long long)a_x[rank_table_index(sx, kx)] * (long long)a_y[rank_table_index(sy, ky)];
    });
    if (missed) atomicAdd(miss, missed);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        acc += (i128)rank_u128(__shfl_xor((unsigned long long)acc, off), __shfl_xor((unsigned long long)((u128)acc >> 64), off));
    if ((threadIdx.x & 63) == 0) w_part[threadIdx.x >> 6] = RankDotPart{(unsigned long long)acc, (long long)(acc >> 64)};
    __syncthreads();
    if (threadIdx.x == 0) {
        u128 t = first ? (u128)0 : rank_u128(part[blockIdx.x].lo, (unsigned long long)part[blockIdx.x].hi);
        for (int w = 0; w < kRankThreads / 64; w++) t += rank_u128(w_part[w].lo, (unsigned long long)w_part[w].hi);
        part[blockIdx.x] = RankDotPart{(unsigned long long)t, (long long)(unsigned long long)(t >> 64)};
    }
}

// the slots, one wave (two's-complement addition: exact in any order)
__global__ __launch_bounds__(64) void k_rank_dot_final(const RankDotPart *__restrict__ part, int n_parts, RankDotPart *__restrict__ out)
{
    u128 t = 0;
    for (int i = threadIdx.x; i < n_parts; i += 64) t += rank_u128(part[i].lo, (unsigned long long)part[i].hi);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        t += rank_u128(__shfl_xor((unsigned long long)t, off), __shfl_xor((unsigned long long)(t >> 64), off));
    if (threadIdx.x == 0) *out = RankDotPart{(unsigned long long)t, (long long)(unsigned long long)(t >> 64)};
}

}  // namespace st
