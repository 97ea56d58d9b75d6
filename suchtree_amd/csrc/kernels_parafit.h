// kernels_parafit.h -- included by suchtree_hip.hip (after kernels_perm.h, whose sorts it uses, and kernels_mantel.h,
// whose row staging and 128-bit folds it follows).
// The device side of st_parafit_codes (layout: parafit_plan.h; the contract: include/suchtree_hip.h).  Link l = (f_l, s_l)
// is relabelled to (f_l, r_p(l)); T_p[l][k] = g_f[f_l][f_k] * g_s[r_p(l)][r_p(k)], the row sum of link l is the sum of
// T_p[l][.] and its record is Link1 = 2 x row sum - T_p[l][l] with the row sum, each in 128 bits.
//
//   k_parafit_expand    once per call: P[l][k] = g_f[f_l][f_k], so the held side is a coalesced stream.
//   k_parafit_relabel*  one sort of the S universe per (permutation, F position with links) by the form its size class
//                       takes (kernels_perm.h), then the images of that position's links into R[p][l].  p = 0 writes s_l.
//   k_parafit_rows      one workgroup per task (link l, permutation p): row R[p][l] of g_s staged in LDS
//                       (mantel_stage_row), lanes stride over k < L: P[l][k] (4 bytes), R[p][k] (2 bytes), one LDS word.
//   k_parafit_wave      L <= 64 and n_s <= 64: one permutation per wave, four per workgroup, g_s and P in LDS at row
//                       stride 65, link l in lane l, R[p][k] from lane k at a wave-uniform k.  Writes the L records and
//                       the permutation's total.
//   k_parafit_fold      per block of permutations: the total of every permutation from its records (row form), and one
//                       wave per link counts Link1_p >= Link1_0 over the block against the saved observation.
//
// Everything is integer arithmetic in two's complement: exact whatever the order, the grid or the chunks.
#pragma once

#include "parafit_plan.h"

namespace st {

static_assert(kParafitThreads == kMantelThreads, "mantel_stage_row strides by kMantelThreads");

__global__ __launch_bounds__(kParafitThreads) void k_parafit_expand(const int *__restrict__ g_f, const unsigned short *__restrict__ link_f, int n_f, int L,
                                                                    int *__restrict__ P)
{
    const int l = blockIdx.y, k = blockIdx.x * kParafitThreads + threadIdx.x;
    if (k < L) P[(size_t)l * (size_t)L + k] = g_f[(size_t)link_f[l] * (size_t)n_f + link_f[k]];
}

struct ParafitGroupDev {
    int stream, begin, count;
};

struct ParafitRelabelArgs {
    const ParafitGroupDev *group;
    const unsigned short *link_s;
    unsigned short *R;                   // the block's rows: R[(p - p0) * L + l]
    unsigned long long seed;
    long long p0, n_tasks;               // task = (p - p0) * n_groups + g
    int n_groups, n_s, L;
};

__global__ __launch_bounds__(256) void k_parafit_relabel_wave(ParafitRelabelArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (wave-uniform)
    if (task >= a.n_tasks) return;
    const long long pb = task / a.n_groups;
    const ParafitGroupDev g = a.group[task - pb * a.n_groups];
    const long long p = a.p0 + pb;
    const unsigned long long key = p != 0 ? perm_sort_wave(perm_stream(a.seed, g.stream, p, 0), a.n_s, lane) : 0;
    for (int l0 = 0; l0 < g.count; l0 += 64) {      // (every lane takes part in the exchange)
        const int l = l0 + lane;
        const int at = l < g.count ? (int)a.link_s[g.begin + l] : 0;
        const int to = p == 0 ? at : (int)(__shfl(key, at) & 0xFFFF);
        if (l < g.count) a.R[(size_t)pb * (size_t)a.L + g.begin + l] = (unsigned short)to;
    }
}

template <int T>
__global__ __launch_bounds__(T) void k_parafit_relabel(ParafitRelabelArgs a)
{
    extern __shared__ unsigned long long perm_keys[];
    const long long task = blockIdx.x;      // (workgroup-uniform)
    const long long pb = task / a.n_groups;
    const ParafitGroupDev g = a.group[task - pb * a.n_groups];
    const long long p = a.p0 + pb;
    const unsigned tid = threadIdx.x;
    if (p != 0) perm_sort_lds<T>(perm_keys, perm_stream(a.seed, g.stream, p, 0), (unsigned)a.n_s, tid);
    for (int l = (int)tid; l < g.count; l += T) {
        const int at = a.link_s[g.begin + l];
        a.R[(size_t)pb * (size_t)a.L + g.begin + l] = (unsigned short)(p == 0 ? at : (int)(perm_keys[at] & 0xFFFF));
    }
}

struct ParafitArgs {
    const int *g_s;                      // n_s x n_s, the base 16-byte aligned
    const int *P;                        // row form: L x L; wave form: not read
    const int *g_f;                      // wave form: n_f x n_f
    const unsigned short *link_f;        // wave form
    const unsigned short *R;             // the block's rows
    ParafitRecord *part;                 // the block's records: entry l * n_perms + (p - p0)
    st_parafit_sum *total;               // wave form: the block's totals, entry p - p0
    long long task0, n_tasks;            // this launch: tasks [task0, task0 + n_tasks) of the block
    unsigned n_perms;
    int n_f, n_s, L;
};

__device__ __forceinline__ ParafitRecord parafit_pack(i128 link, i128 row)
{
    return ParafitRecord{(unsigned long long)link, (long long)(link >> 64), (unsigned long long)row, (long long)(row >> 64)};
}

__global__ __launch_bounds__(kParafitThreads) void k_parafit_rows(ParafitArgs a)
{
    extern __shared__ uint4 parafit_row4[];      // one row of g_s: n_s words
    __shared__ st_parafit_sum w_part[kParafitThreads / 64];
    __shared__ long long diag_s;
    int *lds_row = reinterpret_cast<int *>(parafit_row4);
    const int L = a.L, tid = threadIdx.x;
    const long long t = a.task0 + blockIdx.x;
    const int l = (int)(t / a.n_perms);      // (workgroup-uniform, as is everything the barriers depend on)
    const unsigned short *__restrict__ r = a.R + (size_t)(t - (long long)l * a.n_perms) * (size_t)L;
    mantel_stage_row(lds_row, a.g_s + (size_t)r[l] * (size_t)a.n_s, a.n_s);
    __syncthreads();
    const int *__restrict__ pr = a.P + (size_t)l * (size_t)L;
    i128 row = 0;
#pragma unroll 4
    for (int k = tid; k < L; k += kParafitThreads) {
        const long long term = (long long)pr[k] * (long long)lds_row[r[k]];
        row += term;
        if (k == l) diag_s = term;      // (one lane of the workgroup)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) row += mantel_shfl_xor(row, off);
    if ((tid & 63) == 0) w_part[tid >> 6] = st_parafit_sum{(unsigned long long)row, (long long)(row >> 64)};
    __syncthreads();
    if (tid == 0) {
        i128 s = 0;
        for (int w = 0; w < kParafitThreads / 64; w++) s += mantel_i128(w_part[w].lo, w_part[w].hi);
        a.part[t] = parafit_pack(2 * s - (i128)diag_s, s);
    }
}

__global__ __launch_bounds__(kParafitThreads) void k_parafit_wave(ParafitArgs a)
{
    __shared__ int gs[kParafitWaveMax * kParafitWaveStride];
    __shared__ int ps[kParafitWaveMax * kParafitWaveStride];
    const int L = a.L, n_s = a.n_s, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < n_s * n_s; e += kParafitThreads) gs[(e / n_s) * kParafitWaveStride + e % n_s] = a.g_s[e];
    for (int e = threadIdx.x; e < L * L; e += kParafitThreads)
        ps[(e / L) * kParafitWaveStride + e % L] = a.g_f[(size_t)a.link_f[e / L] * (size_t)a.n_f + a.link_f[e % L]];
    __syncthreads();
    const long long slot = (long long)blockIdx.x * (kParafitThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.n_tasks) return;      // (wave-uniform; no workgroup barrier below)
    const long long t = a.task0 + slot;      // (one item: the task is the block's permutation)
    const bool live = lane < L;
    const int s = live ? (int)a.R[(size_t)t * (size_t)L + lane] : 0;
    const int *srow = gs + s * kParafitWaveStride, *prow = ps + (live ? lane : 0) * kParafitWaveStride;
    i128 row = 0;
    long long diag = 0;
    for (int k = 0; k < L; k++) {
        const int sk = __builtin_amdgcn_readlane(s, k);
        if (live) {
            const long long term = (long long)prow[k] * (long long)srow[sk];
            row += term;
            if (k == lane) diag = term;
        }
    }
    if (live) a.part[(size_t)lane * a.n_perms + (size_t)t] = parafit_pack(2 * row - (i128)diag, row);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) row += mantel_shfl_xor(row, off);
    if (lane == 0) a.total[t] = st_parafit_sum{(unsigned long long)row, (long long)(row >> 64)};
}

// Workgroups [0, n_tot): the total of the block's permutation blockIdx.x from its L row sums (n_tot = n_perms in the row
// form, 0 in the wave form, whose waves wrote their totals).  Workgroups from n_tot: one wave per link l, lanes striding
// over the block's permutations (a link's records are consecutive); the block that starts at p0 = 0 takes the
// observation from record 0 and saves it in obs[l], the others read it there; every block adds its permutations p >= 1
// with Link1_p(l) >= obs[l] to n_ge[l].  No other wave touches obs[l] or n_ge[l], and the blocks follow each other in
// stream order.
__global__ __launch_bounds__(64) void k_parafit_fold(const ParafitRecord *__restrict__ part, int L, unsigned n_perms, long long p0, unsigned n_tot,
                                                     st_parafit_sum *__restrict__ total, st_parafit_sum *__restrict__ obs, long long *__restrict__ n_ge)
{
    if (blockIdx.x < n_tot) {
        i128 s = 0;
        for (int l = threadIdx.x; l < L; l += 64) {
            const ParafitRecord v = part[(size_t)l * n_perms + blockIdx.x];
            s += mantel_i128(v.row_lo, v.row_hi);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += mantel_shfl_xor(s, off);
        if (threadIdx.x == 0) total[blockIdx.x] = st_parafit_sum{(unsigned long long)s, (long long)(s >> 64)};
        return;
    }
    const int l = (int)(blockIdx.x - n_tot);      // (the grid has n_tot + L workgroups)
    const ParafitRecord *__restrict__ rec = part + (size_t)l * n_perms;
    const bool first = p0 == 0;
    const st_parafit_sum seen = first ? st_parafit_sum{rec[0].link_lo, rec[0].link_hi} : obs[l];
    const i128 o = mantel_i128(seen.lo, seen.hi);
    long long count = 0;
    for (unsigned pb = threadIdx.x; pb < n_perms; pb += 64)
        if (!first || pb != 0) count += mantel_i128(rec[pb].link_lo, rec[pb].link_hi) >= o ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (threadIdx.x == 0) {
        if (first) obs[l] = seen;
        n_ge[l] += count;
    }
}

}  // namespace st
