// kernels_hommola.h -- included by suchtree_hip.hip (after kernels_rows.h, kernels_quartets.h and kernels_perm.h).
// The device side of st_hommola_clades_host (layout: hommola_plan.h).  Row (clade, p) is the clade's links relabelled by
// permutation p of each tree's universe; its pair (link j, link i) has x = D_o[q_o(j)][q_o(i)] and y = D_c[q_c(j)][q_c(i)],
// D the float32 distance matrices that the unchanged distance kernels wrote once (SrcGrid), q the relabelled positions.
//
//   k_hommola_relabel*  one sort per (row, side) of the side's universe -- the clade's own leaf range, or the other
//                       tree's leaves -- by the form its size class takes (kernels_perm.h), then every link's position
//                       through sigma into the chunk's buffer of 16-bit position pairs.  p = 0 writes the identity.
//   k_hommola_blocks    one CladePiece per block of ST_CLADE_TILE pairs of a row: two 4-byte gathers for the positions
//                       of links j and i, two for x and y, five multiply-adds (CladeAcc).
//
// Determinism: a block is summed about its own first pair by the order rule of k_row_blocks (kernels_rows.h) -- up to
// kCladeLanePiece pairs by one lane in index order, longer ones by one wave, lane-strided, then the xor butterfly -- so
// a row's pieces are those of st_compare_rows_host on the relabelled ids.  No float atomics.
#pragma once

#include "hommola_plan.h"

namespace st {

constexpr int kHommolaBlockThreads = 256;      // four waves, 64 consecutive blocks each

struct HommolaRelabelArgs {
    const HommolaCladeDev *clade;
    const int *pos;                  // this side's universe position of every link
    unsigned short *rel;             // the chunk's positions: entry 2 * slot + side
    long long row0, n_rows, R;       // rows [row0, row0 + n_rows) of R rows per clade
    long long rel0;                  // global index of row0's first position
    unsigned long long seed;
    int side;                        // 0: the clade tree, over the clade's own leaf range; 1: the other tree
    int n_other;                     // the other tree's universe
    int cls;                         // the size class this launch sorts (PermSortClass); the others return at once
};

struct HommolaTask {
    bool live;
    int n, base, link_begin, links;
    long long p, slot;
    unsigned long long h1;
};

__device__ __forceinline__ HommolaTask hommola_task(const HommolaRelabelArgs &a, long long task)
{
    HommolaTask t{};
    if (task >= a.n_rows) return t;
    const long long row = a.row0 + task, c = row / a.R;
    const HommolaCladeDev d = a.clade[c];
    t.p = row - c * a.R;
    t.n = a.side == 0 ? d.leaf_count : a.n_other;
    t.base = a.side == 0 ? d.leaf_begin : 0;
    t.link_begin = d.link_begin;
    t.links = d.link_count;
    t.slot = d.rel_begin + t.p * d.link_count - a.rel0;
    t.h1 = perm_stream(a.seed, d.node, t.p, a.side);
    t.live = d.link_count >= 2 && perm_sort_class(t.n) == a.cls;
    return t;
}

__global__ __launch_bounds__(256) void k_hommola_relabel_wave(HommolaRelabelArgs a)
{
    const int lane = threadIdx.x & 63;
    const HommolaTask t = hommola_task(a, (long long)blockIdx.x * 4 + (threadIdx.x >> 6));      // (wave-uniform)
    if (!t.live) return;
    const unsigned long long key = t.p != 0 ? perm_sort_wave(t.h1, t.n, lane) : 0;
    for (int l0 = 0; l0 < t.links; l0 += 64) {      // (every lane takes part in the exchange)
        const int l = l0 + lane;
        const int at = l < t.links ? a.pos[t.link_begin + l] - t.base : 0;
        const int to = t.p == 0 ? at : (int)(__shfl(key, at) & 0xFFFF);
        if (l < t.links) a.rel[2 * (t.slot + l) + a.side] = (unsigned short)(t.base + to);
    }
}

template <int T>
__global__ __launch_bounds__(T) void k_hommola_relabel(HommolaRelabelArgs a)
{
    extern __shared__ unsigned long long perm_keys[];
    const HommolaTask t = hommola_task(a, (long long)blockIdx.x);      // (workgroup-uniform)
    if (!t.live) return;
    const unsigned tid = threadIdx.x;
    if (t.p != 0) perm_sort_lds<T>(perm_keys, t.h1, (unsigned)t.n, tid);
    for (int l = (int)tid; l < t.links; l += T) {
        const int at = a.pos[t.link_begin + l] - t.base;
        const int to = t.p == 0 ? at : (int)(perm_keys[at] & 0xFFFF);
        a.rel[2 * (t.slot + l) + a.side] = (unsigned short)(t.base + to);
    }
}

// pair k of a triangle as (col, row), col < row: k = row (row - 1) / 2 + col (the enumeration of SrcTriangle)
__device__ __forceinline__ void hommola_pair(long long k, int &col, int &row)
{
    long long r = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
    if (r * (r - 1) / 2 > k) r--;
    if ((r + 1) * r / 2 <= k) r++;
    row = (int)r;
    col = (int)(k - r * (r - 1) / 2);
}

struct HommolaBlockArgs {
    const HommolaCladeDev *clade;
    const float *mat;                    // the other tree's matrix at 0, the clade matrices behind it
    const unsigned *rel;                 // the chunk's positions: q_c (side 0) in the low half of a word, q_o in the high half
    long long t0, n;                     // global blocks [t0, t0 + n)
    long long R, rel0;
    int n_clades, n_other;
};

struct HommolaGather {
    const float *mo, *mc;
    const unsigned *q;                   // the row's positions, by link
    int n_other, mat_n;

    __device__ __forceinline__ void load(int j, int i, float &x, float &y) const
    {
        const unsigned a = q[j], b = q[i];
        x = mo[(long long)(a >> 16) * n_other + (b >> 16)];
        y = mc[(long long)(a & 0xFFFF) * mat_n + (b & 0xFFFF)];
    }
};

// Wave w takes blocks t0 + 64 w .. t0 + 64 w + 63 in rounds as k_clade_pieces does: lane j sums block j if it is short,
// then the wave sums the long ones together, in block order.  out[j] receives block t0 + j.
__global__ __launch_bounds__(kHommolaBlockThreads) void k_hommola_blocks(HommolaBlockArgs a, CladePiece *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (kHommolaBlockThreads / 64) + (threadIdx.x >> 6);
    const long long j = w * 64 + lane;
    if (w * 64 >= a.n) return;      // (wave-uniform; no workgroup barrier below)
    long long first = 0;
    int len = 0;
    HommolaGather g{};
    if (j < a.n) {
        const long long t = a.t0 + j;
        int lo = 0, hi = a.n_clades - 1;      // the last clade with block_begin <= t
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.clade[mid].block_begin <= t) lo = mid;
            else hi = mid - 1;
        }
        const HommolaCladeDev d = a.clade[lo];
        const long long in = t - d.block_begin, p = in / d.nb, b = in - p * d.nb;
        const long long links = d.link_count, np = links * (links - 1) / 2;
        first = b << kCladeTileShift;
        len = (int)(min((b + 1) << kCladeTileShift, np) - first);
        // (the clade matrix is indexed by universe position: its entry [leaf_begin][leaf_begin] stands at mat_off)
        g = HommolaGather{a.mat, a.mat + d.mat_off - ((long long)d.leaf_begin * d.mat_n + d.leaf_begin),
                          a.rel + (d.rel_begin + p * links - a.rel0), a.n_other, d.mat_n};
    }
    const bool lane_block = len > 0 && len <= kCladeLanePiece;
    if (lane_block) {
        int col, row;
        hommola_pair(first, col, row);
        float x, y;
        g.load(col, row, x, y);
        const float cx = clade_shift(x), cy = clade_shift(y);
        CladeAcc acc;
        for (int i = 0; i < len; i++) {
            g.load(col, row, x, y);
            acc.add(x, y, (double)cx, (double)cy);
            if (++col == row) {
                col = 0;
                row++;
            }
        }
        clade_store(out + j, acc, cx, cy);
    }
    unsigned long long wide = __ballot(len > kCladeLanePiece);
    while (wide) {
        const int b = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const long long wfirst = __shfl(first, b);
        const int wlen = __shfl(len, b);
        HommolaGather wg;
        wg.mo = a.mat;
        wg.mc = reinterpret_cast<const float *>(__shfl((unsigned long long)(uintptr_t)g.mc, b));
        wg.q = reinterpret_cast<const unsigned *>(__shfl((unsigned long long)(uintptr_t)g.q, b));
        wg.n_other = a.n_other;
        wg.mat_n = __shfl(g.mat_n, b);
        int col, row;
        float x, y;
        hommola_pair(wfirst, col, row);
        wg.load(col, row, x, y);
        const float cx = clade_shift(x), cy = clade_shift(y);
        hommola_pair(wfirst + lane, col, row);
        CladeAcc acc;
        for (int i = lane; i < wlen; i += 64) {
            wg.load(col, row, x, y);
            acc.add(x, y, (double)cx, (double)cy);
            col += 64;
            while (col >= row) {
                col -= row;
                row++;
            }
        }
        clade_wave_reduce(acc);
        if (lane == 0) clade_store(out + w * 64 + b, acc, cx, cy);
    }
}

}  // namespace st
