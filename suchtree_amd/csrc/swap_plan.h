// swap_plan.h -- the host-only side of the degree-preserving swap null (st_swap_null_tables, st_dispersion_matrix_swap,
// st_partner_dispersion_swap_host), plain C++17, and what the device shares with it (kernels_swap.h): the draw of a trial,
// the rule that cuts a batch of trials into its conflict-free prefix, the layout of a chain's state.  No GPU calls in
// here (swap_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour sanitizers
// (tests/emu/sanitize_swap.cpp).  The definitions are the contract of include/suchtree_hip.h (st_swap_null_tables).
//
// The link matrix is the table of position sets of the dispersion calls: set r is a row, a position a column, an entry of
// set_pos a link.  Chain p >= 1 starts from the observed links and tries `iterations` swaps of the columns of two links
// drawn from perm_stream(seed, stream, p, 1); a swap that would leave its two rows, or put a column twice into a row, is
// not made.  Rows keep their sizes and columns their degrees, so every chain's table row has the offsets of `sets`.
//
// State of one chain on the device: its table row (n_pos uint16, the chain runs in place in entries sets[0] ..
// sets[n_sets]) and a bit matrix of n_sets rows of `words` 64-bit words (bit c of row r: column c is in row r).  A block
// of chains is bounded by kSwapStateBytes; row_of (int32 per link) is shared by all chains.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "dispersion_plan.h"

namespace st {

constexpr int64_t kSwapStateBytes = (int64_t)4 << 30;      // tables and bit matrices of one block of chains: about a thousand
                                                           // chains of the bench workload (4096 rows over 4096 columns, a million links: 4 MiB each)
constexpr int kSwapBatch = 64;                             // trials a wave draws per step: lane i draws trial t0 + i
constexpr int kSwapThreads = 256;                          // the workgroup of k_swap_chains: four chains

ST_QUARTET_HD uint64_t swap_mulhi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

// trial t of the chain of h1 over L >= 2 links: the two links it draws
ST_QUARTET_HD void swap_draw(uint64_t h1, int64_t t, uint64_t L, int64_t &e1, int64_t &e2)
{
    e1 = (int64_t)swap_mulhi(quartet_mix(h1 + (2 * (uint64_t)t + 1) * kPermGolden), L);
    e2 = (int64_t)swap_mulhi(quartet_mix(h1 + (2 * (uint64_t)t + 2) * kPermGolden), L);
}

// do the trials with rows (a1, a2) and (b1, b2) share a row
ST_QUARTET_HD bool swap_rows_meet(int32_t a1, int32_t a2, int32_t b1, int32_t b2) { return a1 == b1 || a1 == b2 || a2 == b1 || a2 == b2; }

// The prefix rule of a batch of n trials, lane i with rows (r1[i], r2[i]): the first lane one of whose rows is a row of an
// earlier lane, n if there is none.  Lanes below it touch disjoint rows -- disjoint words of the bit matrix and disjoint
// entries -- and every one of them sees the state the serial chain would show it, so they may run at once.  Lane 0 never
// conflicts: the result is at least 1 for n >= 1.  The wave of k_swap_chains evaluates the same predicate over its lanes.
ST_QUARTET_HD int swap_prefix(const int32_t *r1, const int32_t *r2, int n)
{
    for (int i = 1; i < n; i++)
        for (int j = 0; j < i; j++)
            if (swap_rows_meet(r1[i], r2[i], r1[j], r2[j])) return i;
    return n;
}

struct SwapPlan {
    int32_t n_univ = 0;
    int64_t n_pos = 0, n_sets = 0;
    int64_t e0 = 0, L = 0;                // the links: entries [e0, e0 + L) of set_pos
    int64_t iterations = 0;
    int64_t words = 0;                    // 64-bit words of a row of the bit matrix
    int64_t table_bytes = 0;              // one table row: the rows of a block lie back to back
    int64_t chain_bytes = 0;              // table row + bit matrix
    std::vector<int32_t> row_of;          // row_of[e - e0] of link e
};

// ST_OK, or ST_ERR_ARG with `err`.  The set table has been checked (position_sets_args).  Checks, in this order:
// iterations < 0, then a single chain whose state exceeds kSwapStateBytes (with the bytes).
int swap_plan(int32_t n_univ, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t iterations, SwapPlan &P, std::string &err);

// chains a block holds for `rows` chains: as many as kSwapStateBytes allows, at least one; chunk_tasks > 0 bounds it as it
// bounds the sigma block of the taxa-labels calls
int64_t swap_block(const SwapPlan &P, int64_t rows, int64_t chunk_tasks);

// Table row p (n_pos entries) and its accepted trials: the serial chain, trial by trial, then every row sorted.  p = 0, or
// fewer than two links: the observation.  `batched` runs the same trials in the wave's schedule -- batches of kSwapBatch
// cut by swap_prefix -- and adds its steps to *steps (tests: the two forms agree).
void swap_chain_host(const SwapPlan &P, const int32_t *set_pos, const int64_t *sets, uint64_t seed, int32_t stream, int64_t p, uint16_t *row,
                     int64_t *accepted, bool batched = false, int64_t *steps = nullptr);

// the first checks of st_swap_null_tables, in this order: the universe size, negative p_begin, n_perms or stream, the set
// table, then those of swap_plan
int swap_tables_args(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t p_begin, int64_t n_perms,
                     int64_t iterations, int32_t stream, SwapPlan &P, std::string &err);

// The plan of a swap-null dispersion call: dispersion_plan's checks in their order, then swap_plan's; the blocks of
// permutations are cut by swap_block (P.perm_block, P.chunks are rebuilt).
int swap_dispersion_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t permutations,
                         int64_t iterations, int32_t stream, int64_t chunk_tasks, DispersionPlan &P, SwapPlan &S, std::string &err);

// every record of the swap-null call on the host: out[r * rows + p] = dispersion_record over table row p's set r;
// accepted (rows entries) may be NULL
void swap_dispersion_host(const float *D, const DispersionPlan &P, const SwapPlan &S, const int32_t *set_pos, const int64_t *sets, uint64_t seed,
                          int32_t stream, st_dispersion_record *out, int64_t *accepted);

}  // namespace st
