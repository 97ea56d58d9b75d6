// kernels_mantel.h -- included by suchtree_hip.hip (after kernels_dispersion.h, whose k_dispersion_sigma writes the
// sigma rows, and kernels_ranks.h, whose 128-bit folds it follows).
// The device side of st_mantel_codes (layout: mantel_plan.h; the contract: include/suchtree_hip.h).  Permutation p
// relabels the square int32 matrix x through sigma_p; Sxy_p = sum over j < i of x[sigma_p(i)][sigma_p(j)] * y[k(i, j)]
// and, for the partial test, Sxz_p against z, each in 128 bits.
//
//   k_mantel_wave   n <= 64: one permutation per wave, four per workgroup.  The whole of x sits in LDS (row stride 65
//                   words: the 64 rows of one column lie in 64 banks), lane l takes row l, sigma_p(j) comes from lane j
//                   at a wave-uniform j.  The wave writes the permutation's record.
//   k_mantel_rows   n > 64: one workgroup per task (permutation, row pair r).  For each of its rows i = r and n - 1 - r
//                   (the middle row once) it stages row sigma_p(i) of x in LDS -- 16-byte loads from the first aligned
//                   word, up to three words before and after on their own -- then lanes stride over j < i: sigma_p(j)
//                   (2 bytes), y[k(i, j)] and z[k(i, j)] (4 bytes, contiguous for a row), one LDS word at sigma_p(j).
//                   No global gather.  The workgroup writes its task's partial record.  <Gather = true> is the form it
//                   was measured against: the same task without the staging, the word at
//                   sigma_p(j) gathered from the row in global memory.
//   k_mantel_fold   one wave per permutation of the block adds the partial records of its row pairs.
//
// Everything is integer arithmetic in two's complement: exact whatever the order, the grid or the chunks.
#pragma once

#include "mantel_plan.h"

namespace st {

struct MantelArgs {
    const int *x;                        // n x n, the base 16-byte aligned
    const int *y, *z;                    // condensed; z is not read by the <false> forms
    const unsigned short *sigma;         // the block's rows
    st_mantel_sums *part;                // row form: the block's partial records, entry t; wave form: the block's records, entry p - p0
    long long task0, n_tasks;            // this launch: tasks [task0, task0 + n_tasks) of the block
    unsigned n_perms;                    // task t is row pair t / n_perms under row t % n_perms of the block
    int n;
};

__device__ __forceinline__ i128 mantel_shfl_xor(i128 v, int off)
{
    return (i128)rank_u128(__shfl_xor((unsigned long long)v, off), __shfl_xor((unsigned long long)((u128)v >> 64), off));
}

__device__ __forceinline__ st_mantel_sums mantel_pack(i128 xy, i128 xz)
{
    return st_mantel_sums{(unsigned long long)xy, (long long)(xy >> 64), (unsigned long long)xz, (long long)(xz >> 64)};
}

__device__ __forceinline__ i128 mantel_i128(unsigned long long lo, long long hi) { return (i128)rank_u128(lo, (unsigned long long)hi); }

template <bool Z>
__global__ __launch_bounds__(kMantelThreads) void k_mantel_wave(MantelArgs a)
{
    __shared__ int xs[kMantelWaveMax * kMantelWaveStride];
    const int n = a.n, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < n * n; e += kMantelThreads) xs[(e / n) * kMantelWaveStride + e % n] = a.x[e];
    __syncthreads();
    const long long slot = (long long)blockIdx.x * (kMantelThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.n_tasks) return;      // (wave-uniform; no workgroup barrier below)
    const long long t = a.task0 + slot;      // (one item: the task is the block's row)
    const bool live = lane < n;
    const int s = live ? (int)a.sigma[(size_t)t * (size_t)n + lane] : 0;
    const int *row = xs + s * kMantelWaveStride;
    const int k0 = lane * (lane - 1) / 2;
    i128 xy = 0, xz = 0;
    for (int j = 0; j + 1 < n; j++) {
        const int sj = __builtin_amdgcn_readlane(s, j);
        if (live && j < lane) {
            const long long xv = row[sj];
            xy += xv * (long long)a.y[k0 + j];
            if (Z) xz += xv * (long long)a.z[k0 + j];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xy += mantel_shfl_xor(xy, off);
        if (Z) xz += mantel_shfl_xor(xz, off);
    }
    if (lane == 0) a.part[t] = mantel_pack(xy, xz);
}

// row[0 .. n) of x into LDS: src is 4-byte aligned, the words from its first 16-byte boundary go in quads
__device__ __forceinline__ void mantel_stage_row(int *lds, const int *__restrict__ src, int n)
{
    const int tid = threadIdx.x;
    const int head = min((int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u)) & 3u), n);
    if (tid < head) lds[tid] = src[tid];
    const int quads = (n - head) >> 2;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    if (head == 0) {      // (workgroup-uniform)
        uint4 *d4 = reinterpret_cast<uint4 *>(lds);
        for (int q = tid; q < quads; q += kMantelThreads) d4[q] = s4[q];
    } else {
        for (int q = tid; q < quads; q += kMantelThreads) {
            const uint4 v = s4[q];
            int *d = lds + head + 4 * q;
            d[0] = (int)v.x;
            d[1] = (int)v.y;
            d[2] = (int)v.z;
            d[3] = (int)v.w;
        }
    }
    const int tail = head + 4 * quads;
    if (tid < n - tail) lds[tail + tid] = src[tail + tid];
}

template <bool Z, bool Gather>
__global__ __launch_bounds__(kMantelThreads) void k_mantel_rows(MantelArgs a)
{
    extern __shared__ uint4 mantel_row4[];      // one row of x: n words (none in the gather form)
    __shared__ st_mantel_sums w_part[kMantelThreads / 64];
    int *lds_row = reinterpret_cast<int *>(mantel_row4);
    const int n = a.n, tid = threadIdx.x;
    const long long t = a.task0 + blockIdx.x;
    const int r = (int)(t / a.n_perms);      // (workgroup-uniform, as is everything the barriers depend on)
    const unsigned short *__restrict__ sig = a.sigma + (size_t)(t - (long long)r * a.n_perms) * (size_t)n;
    i128 xy = 0, xz = 0;
    const int n_rows = (r == n - 1 - r) ? 1 : 2;
    for (int h = 0; h < n_rows; h++) {
        const int i = h ? n - 1 - r : r;
        if (i == 0) continue;      // (row 0 has no pair j < i)
        const int *__restrict__ row = a.x + (size_t)sig[i] * (size_t)n;
        if (!Gather) {
            if (h) __syncthreads();      // (the row before has been read)
            mantel_stage_row(lds_row, row, n);
            __syncthreads();
            row = lds_row;
        }
        const size_t k0 = (size_t)i * (size_t)(i - 1) / 2;
        const int *__restrict__ yr = a.y + k0;
        const int *__restrict__ zr = Z ? a.z + k0 : nullptr;
#pragma unroll 4
        for (int j = tid; j < i; j += kMantelThreads) {
            const long long xv = row[sig[j]];
            xy += xv * (long long)yr[j];
            if (Z) xz += xv * (long long)zr[j];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xy += mantel_shfl_xor(xy, off);
        if (Z) xz += mantel_shfl_xor(xz, off);
    }
    if ((tid & 63) == 0) w_part[tid >> 6] = mantel_pack(xy, xz);
    __syncthreads();
    if (tid == 0) {
        i128 sxy = 0, sxz = 0;
        for (int w = 0; w < kMantelThreads / 64; w++) {
            sxy += mantel_i128(w_part[w].sxy_lo, w_part[w].sxy_hi);
            sxz += mantel_i128(w_part[w].sxz_lo, w_part[w].sxz_hi);
        }
        a.part[t] = mantel_pack(sxy, sxz);
    }
}

// out[p] of the block's n_perms permutations: the partial records part[r * n_perms + p] over the row pairs r < items
__global__ __launch_bounds__(64) void k_mantel_fold(const st_mantel_sums *__restrict__ part, int items, unsigned n_perms, st_mantel_sums *__restrict__ out)
{
    i128 xy = 0, xz = 0;
    for (int r = threadIdx.x; r < items; r += 64) {
        const st_mantel_sums v = part[(size_t)r * n_perms + blockIdx.x];
        xy += mantel_i128(v.sxy_lo, v.sxy_hi);
        xz += mantel_i128(v.sxz_lo, v.sxz_hi);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xy += mantel_shfl_xor(xy, off);
        xz += mantel_shfl_xor(xz, off);
    }
    if (threadIdx.x == 0) out[blockIdx.x] = mantel_pack(xy, xz);
}

}  // namespace st
