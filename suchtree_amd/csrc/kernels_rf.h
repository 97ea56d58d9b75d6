// kernels_rf.h -- included by suchtree_hip.hip (after kernels_linkage.h).
// The device side of st_rf_tasks (the method, the LDS layout, the key, the extrema and the test of a clade: rf_plan.h; the
// contract: include/suchtree_hip.h).  A task is (tree i, tree j, alignment p); its result is the number of clades of j
// that are clades of i.  Everything is an integer and a task's count is a sum of ones: the grid, the chunk cut and the
// order of the atomic additions give the same numbers.
//
//   k_rf_tasks   one task per workgroup (256 threads, wave64), a workgroup strides over the chunk's tasks.  Per task, in
//                LDS (all of it in the dynamic region, 16-bit entries behind 16 bytes of two int32: rf_lds_bytes):
//                  1. scatter: q[where_j[a[k]]] = where_i[k], k < m -- the one gather of the task; the thread that holds
//                     where_i[k] = 0 notes its position in j;
//                  2. block extrema: a thread reads 8 entries (one 16-byte LDS read), 8 lanes meet with three cross-lane
//                     moves: min and max per block of 64 positions; then the levels of the sparse table, a barrier each
//                     (at most 8);
//                  3. the lanes stride over j's clades (one uint32 each, coalesced): the key of the clade (rf_clade_key:
//                     two table entries and at most 126 entries of q, fewer once the set cannot be a range), a binary
//                     search in tree i's sorted keys (global memory: the tables of a call stay in L2), a ballot and a
//                     popcount per wave, one LDS add per wave, one vector store of the task's count.  With out_count,
//                     a shared clade adds 1 to its own entry and 1 to its match's: vector atomics on global int64.
// Device memory of a call (host_rf.h): 2 m bytes per tree and per alignment row (positions as uint16), 12 bytes per clade
// (its range; its tree's sorted key and index), 4 (n_trees + 1) bytes of offsets, 12 bytes per explicit task, 8 bytes per
// clade of counts when asked for, and two chunks of 4 bytes per task of results.
// Bounds: the host has checked that every row of where and align is a permutation of 0 .. m - 1, every range lies in
// [0, m] with lo < hi, the offsets do not decrease and every task names trees and alignments of the call: q is written
// and read below m, the table below its levels x stride entries (whole blocks [bl, bh) lie below m >> 6), the keys inside
// tree i's list, the counts inside the concatenated list (idx is made by the plan).  Loops run to m, a clade count, the
// levels of the table or the halvings of a search; nothing a loop waits for is written by another thread during it.
#pragma once

#include "rf_plan.h"

namespace st {

struct RfArgs {
    const unsigned short *where;               // n_trees x m: common leaf k -> position
    const unsigned short *align;               // n_align x m
    const int *off;                            // n_trees + 1: a tree's clades in the concatenated list
    const unsigned *range;                     // per clade: lo << 16 | hi
    const unsigned *key;                       // per tree: the canonical keys, increasing
    const int *idx;                            // beside key: the index in the tree's list
    const int *task_i, *task_j, *task_p;       // explicit tasks (task_p may be NULL), or all NULL: the triangle
    long long first;                           // the chunk's first task: an index of the arrays, or a pair of the triangle
    int *out;                                  // the chunk's counts
    unsigned long long *count;                 // per clade, or NULL
    int m, tasks, unrooted;
};

__global__ __launch_bounds__(kRfThreads) void k_rf_tasks(RfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int m = a.m, nb = rf_blocks(m), stride = rf_stride(nb), levels = rf_levels(nb);
    const int tid = threadIdx.x, lane = tid & 63;
    int *meet = reinterpret_cast<int *>(lds);      // [0]: the task's count, [1]: the noted position
    uint16_t *tmin = reinterpret_cast<uint16_t *>(lds + 16), *tmax = tmin + levels * stride, *q = tmax + levels * stride;
    const bool unrooted = a.unrooted != 0;
    for (int t = blockIdx.x; t < a.tasks; t += gridDim.x) {
        int i, j, p = -1;
        if (a.task_i) {
            const long long g = a.first + t;
            i = a.task_i[g];
            j = a.task_j[g];
            if (a.task_p) p = a.task_p[g];
        } else {
            int64_t pi, pj;
            unifrac_pair(a.first + t, pi, pj);
            i = (int)pi;
            j = (int)pj;
        }
        const unsigned short *wi = a.where + (size_t)i * (size_t)m, *wj = a.where + (size_t)j * (size_t)m;
        const unsigned short *al = p >= 0 ? a.align + (size_t)p * (size_t)m : nullptr;
        if (tid == 0) meet[0] = 0;
        for (int k = tid; k < m; k += kRfThreads) {
            const int x = wi[k], y = wj[al ? al[k] : k];
            q[y] = (uint16_t)x;
            if (x == 0) meet[1] = y;
        }
        __syncthreads();
        for (int base = 0; base < m; base += kRfThreads * 8) {      // (the same trips in every lane: the moves below need them all)
            const int e = base + tid * 8;
            int mn = 0xFFFF, mx = 0;
            if (e < m) {
                const uint4 w = *reinterpret_cast<const uint4 *>(q + e);      // (q is padded to 8 entries; those from m on are not used)
                const unsigned v[4] = {w.x, w.y, w.z, w.w};
                for (int h = 0; h < 4; h++) {
                    const int lo16 = (int)(v[h] & 0xFFFFu), hi16 = (int)(v[h] >> 16);
                    if (e + 2 * h < m) {
                        mn = min(mn, lo16);
                        mx = max(mx, lo16);
                    }
                    if (e + 2 * h + 1 < m) {
                        mn = min(mn, hi16);
                        mx = max(mx, hi16);
                    }
                }
            }
            for (int o = 1; o < 8; o <<= 1) {
                mn = min(mn, __shfl_xor(mn, o));
                mx = max(mx, __shfl_xor(mx, o));
            }
            if ((lane & 7) == 0 && e < m) {
                tmin[e >> 6] = (uint16_t)mn;
                tmax[e >> 6] = (uint16_t)mx;
            }
        }
        for (int l = 1; l < levels; l++) {
            __syncthreads();
            const int half = 1 << (l - 1);
            for (int b = tid; b + 2 * half <= nb; b += kRfThreads) {
                const int x = (l - 1) * stride + b;
                tmin[l * stride + b] = min(tmin[x], tmin[x + half]);
                tmax[l * stride + b] = max(tmax[x], tmax[x + half]);
            }
        }
        __syncthreads();
        const int c0 = a.off[j], nj = a.off[j + 1] - c0, k0 = a.off[i], ni = a.off[i + 1] - k0, noted = meet[1];
        const unsigned *keys = a.key + k0;
        int found = 0;
        for (int base = 0; base < nj; base += kRfThreads) {      // (the same trips in every lane: the ballot needs them all)
            const int c = base + tid;
            bool hit = false;
            if (c < nj) {
                const unsigned r = a.range[c0 + c];
                const unsigned key = rf_clade_key(q, tmin, tmax, stride, m, (int)(r >> 16), (int)(r & 0xFFFFu), unrooted, noted);
                if (key != kRfNoKey) {
                    const int at = rf_find(keys, ni, key);
                    hit = at >= 0;
                    if (hit && a.count) {
                        atomicAdd(&a.count[c0 + c], 1ull);
                        atomicAdd(&a.count[k0 + a.idx[k0 + at]], 1ull);
                    }
                }
            }
            found += __popcll(__ballot(hit));
        }
        if (lane == 0 && found) atomicAdd(&meet[0], found);
        __syncthreads();      // (every wave has left q and the table: the next task may write them)
        if (tid == 0) a.out[t] = meet[0];
    }
}

}  // namespace st
