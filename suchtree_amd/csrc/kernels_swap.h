// kernels_swap.h -- included by suchtree_hip.hip (after kernels_dispersion.h, whose table-form task kernels read what this
// one writes).  The device side of the degree-preserving swap null (layout and trial rule: swap_plan.h; the contract:
// include/suchtree_hip.h, st_swap_null_tables).
//
//   k_swap_chains   one wave per chain, four chains per workgroup.  The wave writes the observation into its table row,
//                   builds its bit matrix (a lane owns a row), runs the chain, and reads the rows off the bit matrix in
//                   ascending order into the table row.  Integer arithmetic only.
//
// The chain is serial by definition; the wave runs it in batches that give the serial result exactly.  Lane i draws trial
// t0 + i and looks up its two rows.  A lane conflicts if one of its rows is a row of an earlier lane of the batch
// (swap_rows_meet, the predicate of swap_prefix); lanes below the first conflicting lane f run their trials at once: they
// touch disjoint rows, hence disjoint words of the bit matrix and disjoint 16-bit entries, with plain vector loads and
// stores, no atomics.  t0 advances by f >= 1 (lane 0 never conflicts).  kBatch = 1 is the plain form, one trial per step.
// A step is three dependent round trips to memory: the rows; then, for the lanes that run, their two entries; then the
// four words a swap reads and flips.  kEarly = true is the form with two: every lane loads its entries beside its rows
// and its words before the prefix is known (a lane that will run owns them against every earlier lane of the batch, so
// their values are those of the steps before; what a lane at or above f loaded is dropped).  It is faster while few
// chains run and slower once the chip is full, where the loads of the lanes that do not run cost more than the trip:
// the default is kEarly = false.
//
// Lanes hand state to each other through global memory across steps.  A wave's vector memory instructions execute in
// program order and go through the one L1 of its CU, so a later load sees an earlier store of another lane of the same
// wave; a wavefront-scope fence keeps the compiler from moving loads and stores across a step (as kernels_class.h does
// for LDS).  No workgroup barrier anywhere: the trip counts differ per wave.  Nothing is shared between waves but what all
// only read (set_pos, sets, row_of).
#pragma once

#include "swap_plan.h"

namespace st {

struct SwapChainArgs {
    unsigned short *table;             // chain c of the block: table + c * table_stride, n_pos entries
    unsigned long long *bits;          // chain c's bit matrix: bits + c * bits_stride, n_sets * words words
    const int *set_pos;                // n_pos
    const long long *sets;             // n_sets + 1 offsets
    const int *row_of;                 // L entries: the row of link e0 + e
    long long *accepted;               // per chain of the block
    long long p0;                      // chain c is permutation p0 + c
    unsigned long long seed;
    long long iterations, L, e0, n_pos, table_stride, bits_stride, n_chains;
    int stream, n_sets, words;
};

__device__ __forceinline__ void swap_wave_step()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int kBatch, bool kEarly>
__global__ __launch_bounds__(kSwapThreads) void k_swap_chains(SwapChainArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * (kSwapThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (c >= a.n_chains) return;      // (wave-uniform; no workgroup barrier below)
    const long long p = a.p0 + c;
    unsigned short *const row = a.table + c * a.table_stride;
    unsigned long long *const bits = a.bits + c * a.bits_stride;
    for (long long e = lane; e < a.n_pos; e += 64) row[e] = (unsigned short)a.set_pos[e];      // the observation
    long long accepted = 0;
    if (p != 0 && a.L >= 2 && a.iterations > 0) {
        const long long n_words = (long long)a.n_sets * a.words;
        for (long long w = lane; w < n_words; w += 64) bits[w] = 0;
        swap_wave_step();
        for (int r = lane; r < a.n_sets; r += 64) {      // (positions ascend: a row's words are written once each)
            unsigned long long *const mine = bits + (long long)r * a.words;
            long long at = -1;
            unsigned long long v = 0;
            for (long long e = a.sets[r]; e < a.sets[r + 1]; e++) {
                const int col = a.set_pos[e];
                if ((col >> 6) != at) {
                    if (at >= 0) mine[at] = v;
                    at = col >> 6;
                    v = 0;
                }
                v |= 1ull << (col & 63);
            }
            if (at >= 0) mine[at] = v;
        }
        swap_wave_step();
        const unsigned long long h1 = perm_stream(a.seed, a.stream, p, 1);
        unsigned short *const col = row + a.e0;
        for (long long t0 = 0; t0 < a.iterations;) {
            const long long left = a.iterations - t0;
            const int n = left < kBatch ? (int)left : kBatch;
            const bool live = lane < n;
            int64_t e1 = 0, e2 = 0;
            int r1 = 0, r2 = 0, b = 0, d = 0;
            unsigned long long x1b = 0, x1d = 0, x2b = 0, x2d = 0;      // the four words a swap reads and flips
            auto entries = [&] {
                b = col[e1];
                d = col[e2];
            };
            auto words = [&] {
                const unsigned long long *const w1 = bits + (long long)r1 * a.words, *const w2 = bits + (long long)r2 * a.words;
                x1b = w1[b >> 6];
                x1d = w1[d >> 6];
                x2b = w2[b >> 6];
                x2d = w2[d >> 6];
            };
            if (live) {
                swap_draw(h1, t0 + lane, (unsigned long long)a.L, e1, e2);
                r1 = a.row_of[e1];
                r2 = a.row_of[e2];
                if (kEarly) {      // (a lane that will run owns its entries and words against every earlier lane: the values of the steps before)
                    entries();
                    words();
                }
            }
            int f = n;
            if (kBatch > 1) {      // lanes 0 .. j + 1 are settled once lane j has been compared: stop at the first conflict
                bool conflict = false;
                for (int j = 0; j + 1 < f; j++) {
                    const int j1 = __builtin_amdgcn_readlane(r1, j), j2 = __builtin_amdgcn_readlane(r2, j);
                    conflict |= live && lane > j && swap_rows_meet(r1, r2, j1, j2);
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(conflict);
                    if (m) f = __builtin_ctzll(m);
                }
            }
            if (lane < f) {
                if (!kEarly) {
                    entries();
                    if (r1 != r2 && b != d) words();
                }
                const int wb = b >> 6, wd = d >> 6;
                const unsigned long long bit_b = 1ull << (b & 63), bit_d = 1ull << (d & 63);
                if (r1 != r2 && b != d && !(x1d & bit_d) && !(x2b & bit_b)) {
                    unsigned long long *const w1 = bits + (long long)r1 * a.words, *const w2 = bits + (long long)r2 * a.words;
                    if (wb == wd) {
                        w1[wb] = x1b ^ bit_b ^ bit_d;
                        w2[wb] = x2b ^ bit_b ^ bit_d;
                    } else {
                        w1[wb] = x1b ^ bit_b;
                        w1[wd] = x1d ^ bit_d;
                        w2[wd] = x2d ^ bit_d;
                        w2[wb] = x2b ^ bit_b;
                    }
                    col[e1] = (unsigned short)d;
                    col[e2] = (unsigned short)b;
                    accepted++;
                }
            }
            t0 += f;
            swap_wave_step();
        }
        for (int r = lane; r < a.n_sets; r += 64) {      // the rows read off in order
            const unsigned long long *const mine = bits + (long long)r * a.words;
            long long e = a.sets[r];
            for (int w = 0; w < a.words; w++)
                for (unsigned long long v = mine[w]; v; v &= v - 1) row[e++] = (unsigned short)(w * 64 + __builtin_ctzll(v));
        }
    }
    for (int o = 32; o > 0; o >>= 1) accepted += __shfl_xor(accepted, o);
    if (lane == 0) a.accepted[c] = accepted;
}

}  // namespace st
