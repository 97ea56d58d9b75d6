// kernels_linkage.h -- part of suchtree_hip.hip.  The device side of st_linkage_codes (include/suchtree_hip.h; the cache,
// the candidate and its order: linkage_plan.h).  Two grid passes -- the square int64 S from the codes and the weights, then
// every row's nearest later partner -- and the chain of n - 1 merges as ONE workgroup of kLinkageChainThreads threads.
// The chain synchronises with workgroup barriers only (four per step); it waits on no memory, and every loop has a
// bound that does not depend on data another thread writes.  Per step:
//   1. the arg-min over the cached rows (a slice per thread, a wave's minimum by shuffles, the sixteen waves' through LDS);
//   2. the update of row and column a -- rows a and b are contiguous reads, column a a strided write -- which also sees
//      every candidate of row a's new entry (their minimum: a second workgroup minimum) and, for a row k < a, compares the
//      new S(k, a) with the entry or marks the row for a scan (its partner was a or b; a row between a and b whose
//      partner was b is marked too);
//   3. the marked rows, a wave each: lanes find them 64 rows at a time by ballot, the wave scans the row.
// Lds = the cache (value, partner, size per slot) lives in dynamic LDS, 16 n bytes; else in the global arrays the grid
// passes filled.
#pragma once
#include "linkage_plan.h"

namespace st {

constexpr int kLinkageMarked = -1;      // a row whose partner was merged away: scanned again before the step ends

struct LinkageArgs {
    long long *S;           // n rows of ld
    long long *nn_num;      // the cache as the grid pass left it: the value's numerator,
    int *nn_b;              // the partner (n = none),
    int *size;              // the slot's size (0 = dead)
    int *id;                // the slot's cluster id
    st_linkage_row *out;    // n - 1 rows
    int n, method;
    unsigned ld;            // linkage_row_stride(n)
};

// one element of S per thread: grid (ceil(n / kLinkageExpandThreads), n)
__global__ __launch_bounds__(kLinkageExpandThreads) void k_linkage_expand(const int *__restrict__ codes, const int *__restrict__ weights, int n, int method,
                                                                           unsigned ld, long long *__restrict__ S)
{
    const int i = (int)blockIdx.y, j = (int)(blockIdx.x * kLinkageExpandThreads + threadIdx.x);
    if (j >= n) return;
    long long v = 0;
    if (i != j) {
        const size_t hi = (size_t)(i > j ? i : j), lo = (size_t)(i > j ? j : i);
        v = codes[hi * (hi - 1) / 2 + lo];
        if (method == ST_LINKAGE_AVERAGE && weights) v *= (long long)weights[i] * weights[j];
    }
    S[(size_t)i * ld + (size_t)j] = v;
}

__device__ __forceinline__ LinkageCand linkage_wave_min(LinkageCand c)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const LinkageCand d{__shfl_xor(c.num, o), __shfl_xor(c.den, o), __shfl_xor(c.key, o), __shfl_xor(c.aux, o)};
        if (linkage_before(d, c)) c = d;
    }
    return c;
}

// the minimum over a workgroup of Threads, in every thread; red holds Threads / 64 partials and is free again after
// the caller's next barrier
template <int Threads>
__device__ __forceinline__ LinkageCand linkage_block_min(LinkageCand c, LinkageCand *red)
{
    c = linkage_wave_min(c);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    LinkageCand r = red[0];
#pragma unroll
    for (int w = 1; w < Threads / 64; w++)
        if (linkage_before(red[w], r)) r = red[w];
    return r;
}

// row k's nearest later partner among the active slots, by the lanes of one wave: the result in every lane
__device__ __forceinline__ LinkageCand linkage_scan_row(const long long *__restrict__ row, const int *size, int k, int n, int method, int lane)
{
    const long long s_k = size[k];
    LinkageCand best = linkage_none();
    for (int j = k + 1 + lane; j < n; j += 64) {
        const int s_j = size[j];
        if (!s_j) continue;
        const LinkageCand c{row[j], linkage_den(method, s_k, s_j), j, 0};
        if (linkage_before(c, best)) best = c;
    }
    return linkage_wave_min(best);
}

// the first cache: one workgroup per row, which also gives the slot its size and its id
__global__ __launch_bounds__(kLinkageExpandThreads) void k_linkage_nearest(const long long *__restrict__ S, const int *__restrict__ weights, int n, int method,
                                                                            unsigned ld, long long *__restrict__ nn_num, int *__restrict__ nn_b, int *__restrict__ size,
                                                                            int *__restrict__ id)
{
    __shared__ LinkageCand red[kLinkageExpandThreads / 64];
    const int k = (int)blockIdx.x;
    const long long s_k = weights ? weights[k] : 1;
    const long long *row = S + (size_t)k * ld;
    LinkageCand best = linkage_none();
    for (int j = k + 1 + (int)threadIdx.x; j < n; j += kLinkageExpandThreads) {
        const LinkageCand c{row[j], linkage_den(method, s_k, weights ? weights[j] : 1), j, 0};
        if (linkage_before(c, best)) best = c;
    }
    best = linkage_block_min<kLinkageExpandThreads>(best, red);
    if (threadIdx.x == 0) {
        nn_num[k] = best.num;
        nn_b[k] = best.key == kLinkageNone ? n : best.key;
        size[k] = (int)s_k;
        id[k] = k;
    }
}

template <bool Lds>
__global__ __launch_bounds__(kLinkageChainThreads) void k_linkage_chain(LinkageArgs a)
{
    extern __shared__ long long linkage_lds[];
    __shared__ LinkageCand red_pick[kLinkageChainThreads / 64], red_row[kLinkageChainThreads / 64];
    const size_t ld = a.ld;
    const int n = a.n, method = a.method, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long *nn_num = a.nn_num;
    int *nn_b = a.nn_b, *size = a.size;
    if (Lds) {
        nn_num = linkage_lds;
        nn_b = reinterpret_cast<int *>(linkage_lds + n);
        size = nn_b + n;
        for (int k = tid; k < n; k += kLinkageChainThreads) {
            nn_num[k] = a.nn_num[k];
            nn_b[k] = a.nn_b[k];
            size[k] = a.size[k];
        }
    }
    __syncthreads();
    for (int t = 0; t < n - 1; t++) {
        // 1. the pair of least value, least a, least b
        LinkageCand pick = linkage_none();
        for (int k = tid; k < n; k += kLinkageChainThreads) {
            const int s_k = size[k], b = nn_b[k];
            if (!s_k || (unsigned)b >= (unsigned)n) continue;
            const LinkageCand c{nn_num[k], linkage_den(method, s_k, size[b]), k, b};
            if (linkage_before(c, pick)) pick = c;
        }
        pick = linkage_block_min<kLinkageChainThreads>(pick, red_pick);
        if (pick.key == kLinkageNone) break;      // (two active slots always have a pair: not reached; the same in every thread)
        const int ra = pick.key, rb = pick.aux;
        const long long s_new = (long long)size[ra] + size[rb];
        if (tid == 0) {
            const int ia = a.id[ra], ib = a.id[rb];
            a.out[t] = st_linkage_row{pick.num, pick.den, ia < ib ? ia : ib, ia < ib ? ib : ia, s_new};
            a.id[ra] = n + t;
        }
        // 2. row and column a; row a's new entry; the rows before b that the merge touches
        long long *Sa = a.S + (size_t)ra * ld;
        const long long *Sb = a.S + (size_t)rb * ld;
        LinkageCand best = linkage_none();
        for (int k = tid; k < n; k += kLinkageChainThreads) {
            const int s_k = size[k];
            if (!s_k || k == ra || k == rb) continue;
            const long long v = linkage_merge(method, Sa[k], Sb[k]);
            Sa[k] = v;
            a.S[(size_t)k * ld + (size_t)ra] = v;
            const LinkageCand now{v, linkage_den(method, s_k, s_new), k > ra ? k : ra, 0};
            if (k > ra) {
                if (linkage_before(now, best)) best = now;
                if (k < rb && nn_b[k] == rb) nn_b[k] = kLinkageMarked;
            } else {
                const int b = nn_b[k];
                if (b == ra || b == rb) {
                    nn_b[k] = kLinkageMarked;
                } else {
                    const LinkageCand cur{nn_num[k], linkage_den(method, s_k, size[b]), b, 0};
                    if (linkage_before(now, cur)) {
                        nn_num[k] = v;
                        nn_b[k] = ra;
                    }
                }
            }
        }
        best = linkage_block_min<kLinkageChainThreads>(best, red_row);      // (every thread is past its reads of size[ra], size[rb])
        if (tid == 0) {
            nn_num[ra] = best.num;
            nn_b[ra] = best.key == kLinkageNone ? n : best.key;
            size[ra] = (int)s_new;
            size[rb] = 0;
        }
        __syncthreads();
        // 3. the marked rows, all before b
        for (int base = wave * 64; base < rb; base += kLinkageChainThreads) {
            const int k = base + lane;
            unsigned long long marked = __ballot(k < rb && size[k] && nn_b[k] == kLinkageMarked);
            while (marked) {
                const int row = base + __ffsll((long long)marked) - 1;
                marked &= marked - 1;
                const LinkageCand c = linkage_scan_row(a.S + (size_t)row * ld, size, row, n, method, lane);
                if (lane == 0) {
                    nn_num[row] = c.num;
                    nn_b[row] = c.key == kLinkageNone ? n : c.key;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace st
