// kernels_class.h -- included by suchtree_hip.hip (after kernels_dispersion.h, whose k_dispersion_sigma writes the sigma
// rows, and kernels_mantel.h, whose mantel_stage_row it uses).
// The device side of st_class_sums_codes (layout: class_plan.h; the contract: include/suchtree_hip.h).  Permutation p
// relabels the pairs' classes through sigma_p; out[p][c] = sum over j < i of y[k(i, j)] where the class of the pair
// (sigma_p(i), sigma_p(j)) is c, in 64 bits.
//
//   k_class_expand   n > 64.  The symmetric n x n byte square of the condensed classes, once a call: rows of sliced_stride(n)
//                    bytes (a multiple of 16), the diagonal and the padding kClassNone.
//   k_class_wave     n <= 64: one permutation per wave, four per workgroup.  y (row stride 65 words) and the class square
//                    (row stride 68 bytes: 17 words, odd) sit in LDS; lane l takes row l and s_l = sigma_p(l), sigma_p(j)
//                    comes from lane j at a wave-uniform j, and the lane adds y[l][j] to the wave's accumulator of class
//                    square[s_l][s_j].  Lane c then writes out[p][c].  No partial sums, no fold.
//   k_class_rows     n > 64.  One workgroup per task (row pair r, slice s).  It stages rows r and n - 1 - r of y in LDS --
//                    n - 1 words together, the second row from a quad boundary -- once for the slice; its four waves
//                    then share out the slice's permutations.  For permutation p and row i a wave copies row sigma_p(i)
//                    of the class square into an LDS row of its own (16-byte loads, sliced_stride(n) bytes), then its
//                    lanes stride over j < i: sigma_p(j) (2 bytes, coalesced), the class byte at it in LDS, one LDS
//                    word of y, one 64-bit LDS add to the wave's accumulator of that class.  No global gather: the
//                    first build gathered the byte from the row in global memory and spent its time there (DESIGN.md
//                    section 26).  After both rows lane c writes the partial sum of (p, r, c) and clears its
//                    accumulators.  y comes from memory once a slice.
//                    <Compare = true> is the form it was measured against: no accumulators in
//                    LDS; the wave takes the classes one after the other, each lane adds the y of the pairs whose
//                    class compares equal, and a 64-bit wave reduction leaves the partial sum.
//   k_class_fold     one workgroup per permutation of the block adds the partial sums of its row pairs, class by class.
//
// The accumulators.  kClassCopies 64-bit words per class and wave, word c * kClassCopies + (lane & 3): the lanes of one
// class spread over four addresses in four different bank pairs, so a row that lies in one class -- the worst case --
// meets 16 lanes an address, not 64.  Only the wave itself touches its accumulators: its LDS instructions execute in
// program order, a wavefront-scope fence keeps the compiler from moving the reads across the adds.
//
// Everything is integer arithmetic in two's complement: exact whatever the form, the order, the grid, the chunks or the
// slice.  No global atomics.
#pragma once

#include "class_plan.h"

namespace st {

__global__ __launch_bounds__(kClassThreads) void k_class_expand(const unsigned char *__restrict__ cls, int n, unsigned stride, unsigned char *__restrict__ sq)
{
    const unsigned i = blockIdx.y, j = blockIdx.x * kClassThreads + threadIdx.x;
    if (j >= stride) return;
    unsigned char v = (unsigned char)kClassNone;
    if (j < (unsigned)n && j != i) {
        const size_t a = i > j ? i : j, b = i > j ? j : i;
        v = cls[a * (a - 1) / 2 + b];
    }
    sq[(size_t)i * stride + j] = v;
}

// the wave's accumulators: all zero before and after
__device__ __forceinline__ void class_acc_add(unsigned long long *acc, unsigned c, int lane, int v)
{
    atomicAdd(&acc[c * kClassCopies + (lane & (kClassCopies - 1))], (unsigned long long)(long long)v);
}

// lane c < n_classes: the sum of class c, its accumulators cleared
__device__ __forceinline__ long long class_acc_take(unsigned long long *acc, int lane, int n_classes)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned long long v = 0;
    if (lane < n_classes) {
#pragma unroll
        for (int k = 0; k < kClassCopies; k++) {
            v += acc[lane * kClassCopies + k];
            acc[lane * kClassCopies + k] = 0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return (long long)v;
}

struct ClassWaveArgs {
    const int *y;                        // condensed
    const unsigned char *cls;            // condensed
    const unsigned short *sigma;         // the block's rows
    long long *out;                      // the block's rows of out, entry (p - p0) * n_classes + c
    long long task0, n_tasks;            // this launch: permutations [task0, task0 + n_tasks) of the block
    int n, n_classes;
};

__global__ __launch_bounds__(kClassThreads) void k_class_wave(ClassWaveArgs a)
{
    __shared__ int ys[kClassWaveMax * kClassWaveStride];                 // y[k(i, j)] at i * stride + j
    __shared__ unsigned char cs[kClassWaveMax * kClassWaveBytes];        // the class of (i, j) at i * bytes + j
    __shared__ unsigned long long accs[kClassThreads / 64][kClassMax * kClassCopies];
    const int n = a.n, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = 1 + wave; i < n; i += kClassThreads / 64)
        if (lane < i) {
            const int k = i * (i - 1) / 2 + lane;
            const unsigned char c = a.cls[k];
            ys[i * kClassWaveStride + lane] = a.y[k];
            cs[i * kClassWaveBytes + lane] = c;
            cs[lane * kClassWaveBytes + i] = c;
        }
    unsigned long long *acc = accs[wave];
    for (int e = lane; e < kClassMax * kClassCopies; e += 64) acc[e] = 0;
    __syncthreads();
    const long long slot = (long long)blockIdx.x * (kClassThreads / 64) + wave;
    if (slot >= a.n_tasks) return;      // (wave-uniform; no workgroup barrier below)
    const long long t = a.task0 + slot;
    const bool live = lane < n;
    const int s = live ? (int)a.sigma[(size_t)t * (size_t)n + lane] : 0;
    const int *row = ys + lane * kClassWaveStride;
    const unsigned char *crow = cs + s * kClassWaveBytes;
    for (int j = 0; j + 1 < n; j++) {
        const int sj = __builtin_amdgcn_readlane(s, j);
        if (live && j < lane) {      // (s != sj: the diagonal of cs is never read)
            const unsigned c = crow[sj];
            if (c != (unsigned)kClassNone) class_acc_add(acc, c, lane, row[j]);
        }
    }
    const long long v = class_acc_take(acc, lane, a.n_classes);
    if (lane < a.n_classes) a.out[(size_t)t * (size_t)a.n_classes + lane] = v;
}

struct ClassArgs {
    const int *y;                        // condensed
    const unsigned char *sq;             // the class square, row a at a * stride
    const unsigned short *sigma;         // the block's rows
    long long *part;                     // the block's partial sums, entry ((p - p0) * items + r) * n_classes + c
    long long task0;                     // this launch: tasks [task0, task0 + gridDim.x) of the block
    unsigned n_perms, n_slices, slice;   // task t is row pair t / n_slices under permutations [s * slice, min((s + 1) * slice, n_perms)), s = t % n_slices
    unsigned stride;
    int n, n_classes, items;
};

// the LDS of k_class_rows: rows r and n - 1 - r of y, the second from a quad boundary, then one row of the class square per wave
ST_QUARTET_HD size_t class_y_lds(int n) { return (((size_t)n + 3) * 4 + 15) & ~(size_t)15; }
inline size_t class_row_lds(int32_t n) { return class_y_lds(n) + (kClassThreads / 64) * sliced_stride(n); }

// row `src` of the class square (stride bytes, 16-byte aligned) into the wave's LDS row: the wave alone reads and writes it
__device__ __forceinline__ void class_stage_row(uint4 *dst, const unsigned char *__restrict__ src, unsigned stride, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the row before has been read)
    __builtin_amdgcn_wave_barrier();
    const uint4 *__restrict__ s4 = reinterpret_cast<const uint4 *>(src);
    for (unsigned q = lane; q < stride / 16; q += 64) dst[q] = s4[q];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <bool Compare>
__global__ __launch_bounds__(kClassThreads) void k_class_rows(ClassArgs a)
{
    extern __shared__ uint4 class_row4[];      // the row pair of y, then the waves' rows of the class square
    __shared__ unsigned long long accs[kClassThreads / 64][kClassMax * kClassCopies];
    int *lds_row = reinterpret_cast<int *>(class_row4);
    const int n = a.n, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long t = a.task0 + blockIdx.x;
    const int r = (int)(t / a.n_slices);      // (workgroup-uniform)
    const unsigned p_begin = (unsigned)(t - (long long)r * a.n_slices) * a.slice, p_end = min(p_begin + a.slice, a.n_perms);
    const int n_rows = (r == n - 1 - r) ? 1 : 2;
    const int at1 = (r + 3) & ~3;      // (the second row's word offset in LDS: at1 + n - 1 - r < n + 3)
    for (int h = 0; h < n_rows; h++) {
        const int i = h ? n - 1 - r : r;
        if (i > 0) mantel_stage_row(lds_row + (h ? at1 : 0), a.y + (size_t)i * (size_t)(i - 1) / 2, i);      // (row 0 has no pair j < i)
    }
    uint4 *crow4 = class_row4 + (class_y_lds(n) + (size_t)wave * a.stride) / 16;
    const unsigned char *crow = reinterpret_cast<const unsigned char *>(crow4);
    unsigned long long *acc = accs[wave];
    if (!Compare)
        for (int e = lane; e < kClassMax * kClassCopies; e += 64) acc[e] = 0;
    __syncthreads();
    for (unsigned p = p_begin + wave; p < p_end; p += kClassThreads / 64) {
        const unsigned short *__restrict__ sig = a.sigma + (size_t)p * (size_t)n;
        long long *__restrict__ part = a.part + ((size_t)p * (size_t)a.items + (size_t)r) * (size_t)a.n_classes;
        for (int h = 0; h < n_rows; h++) {
            const int i = h ? n - 1 - r : r;
            const int *yr = lds_row + (h ? at1 : 0);
            if (i > 0) class_stage_row(crow4, a.sq + (size_t)__builtin_amdgcn_readfirstlane((int)sig[i]) * a.stride, a.stride, lane);
            if (!Compare) {
#pragma unroll 4
                for (int j = lane; j < i; j += 64) {
                    const unsigned c = crow[sig[j]];
                    if (c != (unsigned)kClassNone) class_acc_add(acc, c, lane, yr[j]);
                }
            } else {
                for (int c = 0; c < a.n_classes; c++) {
                    long long sum = 0;
#pragma unroll 4
                    for (int j = lane; j < i; j += 64)
                        if ((int)crow[sig[j]] == c) sum += yr[j];
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
                    if (lane == 0) part[c] = h ? part[c] + sum : sum;      // (the same lane, in program order)
                }
            }
        }
        if (!Compare) {
            const long long v = class_acc_take(acc, lane, a.n_classes);
            if (lane < a.n_classes) part[lane] = v;
        }
    }
}

// out[p][0 .. n_classes) of the block's permutations: the partial sums part[(p * items + r) * n_classes + c] over the row pairs r
__global__ __launch_bounds__(kClassThreads) void k_class_fold(const long long *__restrict__ part, int items, int n_classes, long long *__restrict__ out)
{
    __shared__ long long w_sum[kClassThreads / 64][kClassMax];
    static_assert(kClassMax == 64, "one class per lane");
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long *__restrict__ mine = part + (size_t)blockIdx.x * (size_t)items * (size_t)n_classes;
    long long sum = 0;
    if (c < n_classes)
        for (int r = w; r < items; r += kClassThreads / 64) sum += mine[(size_t)r * (size_t)n_classes + c];
    w_sum[w][c] = sum;
    __syncthreads();
    if (w == 0 && c < n_classes) {
        for (int k = 1; k < kClassThreads / 64; k++) sum += w_sum[k][c];
        out[(size_t)blockIdx.x * (size_t)n_classes + c] = sum;
    }
}

}  // namespace st
