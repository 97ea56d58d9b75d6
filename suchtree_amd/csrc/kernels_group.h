// kernels_group.h -- included by suchtree_hip.hip (after kernels_dispersion.h, whose k_dispersion_sigma writes the sigma
// rows, and kernels_mantel.h, whose mantel_stage_row it uses).
// The device side of st_group_sums_codes (layout: group_plan.h; the contract: include/suchtree_hip.h).  Permutation p
// relabels the n objects' group labels through sigma_p; out[p][h] = sum over j < i with both relabelled labels h of
// y[k(i, j)], in 64 bits.
//
//   k_group_wave      n <= 64: one permutation per wave, four per workgroup.  The whole of y sits in LDS as a square (row
//                     stride 65 words: the 64 rows of one column lie in 64 banks); lane l takes row l and the label
//                     g_l = group[sigma_p(l)], the label of column j comes from lane j at a wave-uniform j, and the lane
//                     adds y where the two agree.  Lane h then adds the row sums of the lanes whose label is h, again
//                     lane by lane, and writes out[p][h] -- 64 columns a pass.  No relabel, no partial records, no fold.
//                     The row form below leaves 48 lanes of every wave idle at this size and was measured at twice
//                     the Mantel wave form's time.
//   k_group_relabel   n > 64.  G[p][j] = group[sigma_p(j)] as bytes for the block's permutations, rows of sliced_stride(n) bytes
//                     (a multiple of 16: a row starts 16-byte aligned), the padding zero.
//   k_group_rows      n > 64.  One workgroup per task (row pair r, slice s).  For each of its rows i = r and n - 1 - r (the middle
//                     row once) it stages y[k0 .. k0 + i) in LDS at word j, once for the slice; its four waves then share
//                     out the slice's permutations.  For permutation p a wave reads g = G[p][i] (wave-uniform), its
//                     lanes stride over j in quads -- one aligned word of G[p], one 16-byte LDS read of y, four byte
//                     compares, a 64-bit conditional add -- and after a 64-bit wave reduction lane 0 writes the partial
//                     record (sum, g) of (row, permutation).  No global gather, no multiply; y comes from memory once a
//                     slice.
//   k_group_fold      one workgroup per permutation of the block adds the rows' partial records into 256 int64 LDS
//                     accumulators by group (LDS integer atomics: any order, the same sums) and writes the row of out.
//
// Everything is integer arithmetic in two's complement: exact whatever the form, the order, the grid, the chunks or the
// slice.
#pragma once

#include "group_plan.h"

namespace st {

struct GroupArgs {
    const int *y;                        // condensed
    const unsigned char *G;              // the block's relabelled labels, row p - p0 at (p - p0) * stride
    GroupPart *part;                     // the block's partial records, entry (p - p0) * n + i
    long long task0;                     // this launch: tasks [task0, task0 + gridDim.x) of the block
    unsigned n_perms, n_slices, slice;   // task t is row pair t / n_slices under permutations [s * slice, min((s + 1) * slice, n_perms)), s = t % n_slices
    unsigned stride;
    int n;
};

__global__ __launch_bounds__(kGroupThreads) void k_group_relabel(const unsigned short *__restrict__ sigma, const unsigned char *__restrict__ group, int n,
                                                                  unsigned stride, unsigned char *__restrict__ G)
{
    const size_t p = blockIdx.x;      // one workgroup per permutation of the block
    for (unsigned j = threadIdx.x; j < stride; j += kGroupThreads)
        G[p * stride + j] = j < (unsigned)n ? group[sigma[p * (size_t)n + j]] : (unsigned char)0;
}

struct GroupWaveArgs {
    const int *y;                        // condensed
    const unsigned char *group;          // the n labels as uploaded
    const unsigned short *sigma;         // the block's rows
    long long *out;                      // the block's rows of out, entry (p - p0) * n_groups + h
    long long task0, n_tasks;            // this launch: permutations [task0, task0 + n_tasks) of the block
    int n, n_groups;
};

__global__ __launch_bounds__(kGroupThreads) void k_group_wave(GroupWaveArgs a)
{
    __shared__ int ys[kGroupWaveMax * kGroupWaveStride];      // y[k(i, j)] at i * stride + j
    const int n = a.n, lane = threadIdx.x & 63;
    for (int i = 1 + (int)(threadIdx.x >> 6); i < n; i += kGroupThreads / 64)
        if (lane < i) ys[i * kGroupWaveStride + lane] = a.y[i * (i - 1) / 2 + lane];
    __syncthreads();
    const long long slot = (long long)blockIdx.x * (kGroupThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.n_tasks) return;      // (wave-uniform; no workgroup barrier below)
    const long long t = a.task0 + slot;
    const bool live = lane < n;
    const int g = live ? (int)a.group[a.sigma[(size_t)t * (size_t)n + lane]] : -1;      // (-1: no label)
    const int *row = ys + lane * kGroupWaveStride;
    long long sum = 0;      // row `lane`: over j < lane with the lane's label
    for (int j = 0; j + 1 < n; j++) {
        const int gj = __builtin_amdgcn_readlane(g, j);
        if (j < lane && gj == g) sum += row[j];
    }
    const int lo = (int)(unsigned)(unsigned long long)sum, hi = (int)(unsigned)((unsigned long long)sum >> 32);
    long long *__restrict__ out = a.out + (size_t)t * (size_t)a.n_groups;
    for (int h = lane; h < a.n_groups + lane; h += 64) {      // (wave-uniform trips: readlane below needs every lane there)
        long long col = 0;
        for (int j = 1; j < n; j++) {
            const long long sj = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, j) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, j));
            if (__builtin_amdgcn_readlane(g, j) == h) col += sj;
        }
        if (h < a.n_groups) out[h] = col;
    }
}

__global__ __launch_bounds__(kGroupThreads) void k_group_rows(GroupArgs a)
{
    extern __shared__ uint4 group_row4[];      // one row of y: n words, rounded up to a quad
    int *lds_row = reinterpret_cast<int *>(group_row4);
    const int n = a.n, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long t = a.task0 + blockIdx.x;
    const int r = (int)(t / a.n_slices);      // (workgroup-uniform, as is everything the barriers depend on)
    const unsigned p_begin = (unsigned)(t - (long long)r * a.n_slices) * a.slice, p_end = min(p_begin + a.slice, a.n_perms);
    const int n_rows = (r == n - 1 - r) ? 1 : 2;
    for (int h = 0; h < n_rows; h++) {
        const int i = h ? n - 1 - r : r;
        if (i == 0) continue;      // (row 0 has no pair j < i)
        if (h) __syncthreads();      // (the row before has been read)
        mantel_stage_row(lds_row, a.y + (size_t)i * (size_t)(i - 1) / 2, i);
        __syncthreads();
        const int quads = (i + 3) >> 2;
        for (unsigned p = p_begin + wave; p < p_end; p += kGroupThreads / 64) {
            const unsigned char *__restrict__ Gp = a.G + (size_t)p * a.stride;
            const unsigned g = (unsigned)__builtin_amdgcn_readfirstlane((int)Gp[i]);
            const unsigned g4 = g * 0x01010101u;
            const unsigned *__restrict__ Gw = reinterpret_cast<const unsigned *>(Gp);
            long long sum = 0;
            for (int q = lane; q < quads; q += 64) {
                const unsigned x = Gw[q] ^ g4;      // (byte b is 0 where G[p][4 q + b] == g)
                const uint4 v = group_row4[q];
                const int j = 4 * q;
                if ((x & 0x000000FFu) == 0) sum += (int)v.x;      // (j < i: q < quads)
                if ((x & 0x0000FF00u) == 0 && j + 1 < i) sum += (int)v.y;
                if ((x & 0x00FF0000u) == 0 && j + 2 < i) sum += (int)v.z;
                if ((x & 0xFF000000u) == 0 && j + 3 < i) sum += (int)v.w;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
            if (lane == 0) a.part[(size_t)p * (size_t)n + (size_t)i] = GroupPart{sum, (int)g, 0};
        }
    }
}

// out[p][0 .. n_groups) of the block's permutations: the partial records part[p * n + i] over the rows 1 <= i < n
__global__ __launch_bounds__(kGroupThreads) void k_group_fold(const GroupPart *__restrict__ part, int n, int n_groups, long long *__restrict__ out)
{
    __shared__ unsigned long long acc[kGroupMax];
    static_assert(kGroupMax == kGroupThreads, "one accumulator per thread");
    acc[threadIdx.x] = 0;
    __syncthreads();
    const GroupPart *__restrict__ mine = part + (size_t)blockIdx.x * (size_t)n;
    for (int i = 1 + threadIdx.x; i < n; i += kGroupThreads) {
        const GroupPart v = mine[i];
        atomicAdd(&acc[v.g], (unsigned long long)v.sum);
    }
    __syncthreads();
    if ((int)threadIdx.x < n_groups) out[(size_t)blockIdx.x * (size_t)n_groups + threadIdx.x] = (long long)acc[threadIdx.x];
}

}  // namespace st
