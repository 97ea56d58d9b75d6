// kernels_unifrac_null.h -- included by suchtree_hip.hip (after kernels_unifrac.h).
// The device side of st_unifrac_null_host and st_unifrac_null_depths (layout: unifrac_null_plan.h; the contract:
// include/suchtree_hip.h).  Per block of permutations the sigma rows come from k_dispersion_sigma; then, over the int64
// depths and the range-minimum table of kernels_unifrac.h, with no float arithmetic:
//
//   k_null_unifrac_sets   one (set, p) task per workgroup of one wave.  The members' images sigma_p[s] set their bits in
//                         an LDS bitmap of n <= 16384 bits (an LDS atomic OR: two members may share a word).  The lanes
//                         then take 64 words a pass: a popcount prefix over the wave gives a word's first rank, a lane
//                         reads its word's positions off in ascending order, finds each one's successor (the next bit
//                         of the word, or the first bit of the next word that is not empty) and adds q(d[x]) minus the
//                         range minimum up to the successor.  O(n / 64 + k), no sort.  Where pair results are wanted
//                         the ordered positions go to the set's offsets in row p of the block's relabelled table, 16
//                         bits each.  An int64 butterfly finishes PD and lane 0 stores it.
//   k_null_unifrac_lane   one (pair, p) task per lane over a rectangle of n_pairs consecutive pairs and n_p consecutive
//                         rows, pair fastest: the lanes of a wave share row p of the table (the lists of neighbouring
//                         sets lie behind one another in it) and mostly set i; a lane stores its result at pair x
//                         n_perms + row, the order of the caller's array.  unifrac_merge of kernels_unifrac.h; a task
//                         of more than lane_max positions goes to the launch's heavy list, as in k_unifrac_lane.
//                         (Measured against row fastest, where a wave walks 64 rows of one pair: 1.29 against 1.61 ms
//                         per launch of 2^20 tasks, profiles/unifrac_null_r22.log.)
//   k_null_unifrac_wave   the fixed grid of k_unifrac_wave drains the list: unifrac_successor over the two lists of row p.
// Every result cell is written once.  Table rows are written by the set tasks of a block before any pair task of it is
// launched (stream order).
#pragma once

#include "unifrac_null_plan.h"

namespace st {

constexpr int kUnifracNullWords = kPermMaxUniverse / 64;      // the bitmap: 2 KiB

struct UnifracNullArgs {
    const int64_t *d_q;              // n depths
    const int64_t *table;            // levels x m, level 0 = h_q
    const unsigned short *sigma;     // the block's rows: n_perms x n
    const int *set_pos;
    const int64_t *sets;             // n_sets + 1 offsets into set_pos
    unsigned short *relabelled;      // the block's table: n_perms x n_tab, a row laid out as set_pos (NULL: not written)
    int64_t *out;                    // this launch's results: entry `slot`
    unsigned *heavy;                 // the pair launch's heavy list: up to `count` result indices ...
    unsigned *n_heavy;               // ... and its length
    long long m, n_tab;
    long long task0;                 // set launches: the first task of the block, set * n_perms + row
    long long pair_first;            // pair launches: the triangle index of the first pair ...
    unsigned n_pairs, p_first;       // ... of n_pairs, and the first row of count / n_pairs (all n_perms rows, or one pair)
    unsigned count, n_perms;         // tasks of the launch; rows of the block
    int n, lane_max, want_pd;
};

__global__ __launch_bounds__(64) void k_null_unifrac_sets(UnifracNullArgs a)
{
    __shared__ unsigned long long bitmap[kUnifracNullWords];
    const unsigned lane = threadIdx.x;
    const long long t = a.task0 + blockIdx.x, r = t / a.n_perms;
    const unsigned p = (unsigned)(t - r * a.n_perms);
    const long long b = a.sets[r], e = a.sets[r + 1];
    const int words = (a.n + 63) >> 6, none = 0x7FFFFFFF;
    for (int w = lane; w < words; w += 64) bitmap[w] = 0;
    __syncthreads();
    const unsigned short *sig = a.sigma + (size_t)p * (size_t)a.n;
    for (long long x = b + lane; x < e; x += 64) {
        const unsigned q = sig[a.set_pos[x]];
        atomicOr(&bitmap[q >> 6], 1ull << (q & 63));
    }
    __syncthreads();
    unsigned short *row = a.relabelled ? a.relabelled + (size_t)p * (size_t)a.n_tab + b : nullptr;
    int64_t sum = 0;
    unsigned base = 0;
    for (int w0 = 0; w0 < words; w0 += 64) {      // (workgroup-uniform: every lane takes part in the prefix)
        const int w = w0 + (int)lane;
        unsigned long long bits = w < words ? bitmap[w] : 0;
        const unsigned c = (unsigned)__popcll(bits);
        unsigned upto = c;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(upto, o);
            if ((int)lane >= o) upto += v;
        }
        unsigned rank = base + upto - c;
        base += __shfl(upto, 63);
        if (!bits) continue;
        int after = none;      // the first member past this word
        for (int v = w + 1; v < words; v++) {
            const unsigned long long nb = bitmap[v];
            if (nb) {
                after = v * 64 + __builtin_ctzll(nb);
                break;
            }
        }
        while (bits) {
            const int x = w * 64 + __builtin_ctzll(bits);
            bits &= bits - 1;
            const int next = bits ? w * 64 + __builtin_ctzll(bits) : after;
            if (a.want_pd) {
                sum += a.d_q[x];
                if (next != none) sum -= unifrac_rmq(a.table, a.m, x, next);
            }
            if (row) row[rank] = (unsigned short)x;
            rank++;
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) a.out[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kUnifracThreads) void k_null_unifrac_lane(UnifracNullArgs a)
{
    const unsigned slot = blockIdx.x * kUnifracThreads + threadIdx.x;
    if (slot >= a.count) return;
    const unsigned row = slot / a.n_pairs, pair = slot - row * a.n_pairs, at = pair * a.n_perms + row;
    int64_t i, j;
    unifrac_pair((int64_t)(a.pair_first + pair), i, j);
    const long long pa = a.sets[j], pb = a.sets[i], ea = a.sets[j + 1], eb = a.sets[i + 1];
    if ((ea - pa) + (eb - pb) > a.lane_max) {
        a.heavy[atomicAdd(a.n_heavy, 1u)] = at;
        return;
    }
    a.out[at] = unifrac_merge(a.d_q, a.table, a.m, a.relabelled + (size_t)(a.p_first + row) * (size_t)a.n_tab, pa, ea, pb, eb);
}

__global__ __launch_bounds__(kUnifracThreads) void k_null_unifrac_wave(UnifracNullArgs a)
{
    const unsigned lane = threadIdx.x & 63, waves = gridDim.x * (kUnifracThreads / 64);
    const unsigned n_heavy = *a.n_heavy;      // (written by the launch before this one)
    for (unsigned w = blockIdx.x * (kUnifracThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); w < n_heavy; w += waves) {
        const unsigned at = (unsigned)__builtin_amdgcn_readfirstlane((int)a.heavy[w]), pair = at / a.n_perms, row = at - pair * a.n_perms;
        int64_t i, j;
        unifrac_pair((int64_t)(a.pair_first + pair), i, j);
        int64_t sum = unifrac_successor(a.d_q, a.table, a.m, a.relabelled + (size_t)(a.p_first + row) * (size_t)a.n_tab, a.sets[j], a.sets[j + 1],
                                        a.sets[i], a.sets[i + 1], false, lane);
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) a.out[at] = sum;
    }
}

}  // namespace st
