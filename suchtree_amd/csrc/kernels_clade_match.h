// kernels_clade_match.h -- included by suchtree_hip.hip (after kernels_unifrac.h).
// The device side of st_clade_match (ranges, the distance, the key and the windows: clade_match_plan.h; the contract:
// include/suchtree_hip.h).  Row a of tree A is a range [lo, hi) of A's leaf positions; pos_b takes those to B's
// positions, where every candidate is a range again, so |a n b| is a difference of two ranks in the set pos_b[lo .. hi).
// Everything is an integer and a row's result is the minimum of a key that no two candidates share: the windows, the
// grid and the chunk cut give the same three numbers.
//
//   k_clade_match   one row per workgroup, a workgroup strides over the chunk's rows.  Per row, in LDS (all of it in the
//                   dynamic region: 12 bytes per 64 leaves and 64 bytes where the waves meet):
//                     1. the bitmap of m bits (and one word of padding, so rank(m) reads a word) is cleared;
//                     2. the bits pos_b[lo .. hi) are set (a 32-bit LDS atomic or per leaf);
//                     3. one uint32 running count per 64-bit word: a thread sums the popcounts of its run of words, the
//                        wave scans the sums with cross-lane moves, the waves meet in LDS, the thread writes its run.
//                        rank(x) = count[x >> 6] + popcount(word[x >> 6] & ((1 << (x & 63)) - 1));
//                     4. the lanes stride over B's candidates (sorted by size; lo, hi and index are three coalesced
//                        reads of arrays that stay in L2): i = rank(hi) - rank(lo), delta, the key delta << 32 | index,
//                        a per-lane minimum that carries i.  First the row's windows; where they hold nothing below
//                        p - 1, all candidates;
//                     5. the wave reduces (key, i) with cross-lane moves, the waves meet in LDS, lane 0 stores the
//                        row's three int32 (vector stores).
// Bounds: the host has checked that pos_b is a permutation of 0 .. m - 1 and every range lies in [0, m], so a bit index
// is below m and a rank argument at most m, whose word is the padding word at the latest; the windows are indices of
// the sorted list, made by the plan.
#pragma once

#include "clade_match_plan.h"

namespace st {

struct CladeMatchArgs {
    const int *pos_b;                    // m: A position -> B position
    const int *a_lo, *a_hi;              // every row of the call
    const int *win;                      // 4 per row (CladeMatchPlan::win)
    const int *b_lo, *b_hi, *b_idx;      // n_b candidates by size, and their index in B's list
    int *out;                            // this chunk's results: distance, match, intersection of row r at 3 r
    int m, n_b;
    int row_begin, rows;                 // the chunk
    int unrooted;
};

// the minimum key of the workgroup, with its i, in every thread; `meet` is the 64 bytes of clade_match_lds_tail
__device__ __forceinline__ void clade_match_reduce(unsigned long long &key, int &i, char *meet)
{
    unsigned long long *wave_key = reinterpret_cast<unsigned long long *>(meet);
    int *wave_i = reinterpret_cast<int *>(meet + 32);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_xor(key, o);
        const int v = __shfl_xor(i, o);
        if (k < key) {
            key = k;
            i = v;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wave_key[wave] = key;
        wave_i[wave] = i;
    }
    __syncthreads();
    for (int q = 0; q < kCladeMatchThreads / 64; q++)
        if (wave_key[q] < key) {
            key = wave_key[q];
            i = wave_i[q];
        }
    __syncthreads();      // (the slots are free again)
}

__global__ __launch_bounds__(kCladeMatchThreads) void k_clade_match(CladeMatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int W = clade_match_words(a.m), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long *word = reinterpret_cast<unsigned long long *>(lds);
    unsigned *half = reinterpret_cast<unsigned *>(lds);
    unsigned *count = reinterpret_cast<unsigned *>(lds + (size_t)W * 8);
    char *meet = lds + clade_match_lds_tail(a.m);
    unsigned *wave_sum = reinterpret_cast<unsigned *>(meet + 48);
    const int per = (W + kCladeMatchThreads - 1) / kCladeMatchThreads;      // a thread's run of words in the scan
    const int w0 = min(tid * per, W), w1 = min(w0 + per, W);
    const bool unrooted = a.unrooted != 0;
    for (int r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const int row = a.row_begin + r, lo = a.a_lo[row], hi = a.a_hi[row], sa = hi - lo;
        for (int w = tid; w < W; w += kCladeMatchThreads) word[w] = 0;
        __syncthreads();
        for (int k = lo + tid; k < hi; k += kCladeMatchThreads) {
            const unsigned x = (unsigned)a.pos_b[k];
            atomicOr(&half[x >> 5], 1u << (x & 31));      // (little endian: bit x & 63 of word x >> 6)
        }
        __syncthreads();
        unsigned mine = 0;
        for (int w = w0; w < w1; w++) mine += (unsigned)__popcll(word[w]);
        unsigned inc = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        unsigned base = inc - mine;
        for (int q = 0; q < wave; q++) base += wave_sum[q];
        for (int w = w0; w < w1; w++) {
            count[w] = base;
            base += (unsigned)__popcll(word[w]);
        }
        __syncthreads();
        unsigned long long best = kCladeMatchNoKey;
        int best_i = 0;
        auto rank = [&](int x) {
            const int w = x >> 6;
            return (int)(count[w] + (unsigned)__popcll(word[w] & ((1ull << (x & 63)) - 1ull)));
        };
        auto scan = [&](int c0, int c1) {
            for (int c = c0 + tid; c < c1; c += kCladeMatchThreads) {
                const int bl = a.b_lo[c], bh = a.b_hi[c], i = rank(bh) - rank(bl);
                const unsigned long long key = clade_match_key(clade_match_delta(sa, bh - bl, i, a.m, unrooted), a.b_idx[c]);
                if (key < best) {
                    best = key;
                    best_i = i;
                }
            }
        };
        const int *w = a.win + (size_t)row * 4;
        scan(w[0], w[1]);
        scan(w[2], w[3]);
        clade_match_reduce(best, best_i, meet);
        if (best == kCladeMatchNoKey || (int)(best >> 32) >= clade_match_bound(sa, a.m, unrooted)) {      // (the same in every thread)
            scan(0, a.n_b);
            clade_match_reduce(best, best_i, meet);
        }
        if (tid == 0) {
            int *out = a.out + (size_t)r * 3;
            out[0] = best == kCladeMatchNoKey ? -1 : (int)(best >> 32);
            out[1] = best == kCladeMatchNoKey ? -1 : (int)(best & 0xFFFFFFFFu);
            out[2] = best_i;
        }
    }
}

}  // namespace st
