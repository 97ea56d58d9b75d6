// hommola_plan.h -- the host-only side of Hommola's permutation test for many clades at once (st_hommola_clades_host),
// plain C++17, and the clade table the device shares with it (kernels_hommola.h); the permutation of a row is
// keyed_perm.h's.  No GPU calls in here (hommola_plan.cpp): the "not gpu" tests run it under the
// address / undefined-behaviour sanitizers (tests/emu/sanitize_hommola.cpp).  The definitions are the contract of
// include/suchtree_hip.h (st_hommola_clades_host).
//
// Layout.  Row r = clade * (permutations + 1) + p is clade `clade` under permutation p (p = 0: the links as they are).
// A row of L links has L (L - 1) / 2 pairs, cut into blocks of ST_CLADE_TILE pairs from its first pair; blocks are
// numbered row after row, and a chunk is a range of whole blocks.  The maximal clade ranges (those inside no other
// range of the call) each own one square float32 matrix of clade-tree distances behind the other tree's matrix; a
// nested clade reads its part of the maximal matrix around it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "compare_plan.h"
#include "keyed_perm.h"

namespace st {

// what the device reads of one clade (and the host of its rows and blocks); a sentinel closes the table
struct HommolaCladeDev {
    long long block_begin;      // global index of the first block of the clade's row 0 (the sentinel: the block count)
    long long rel_begin;        // global index of the first relabelled position of the clade's row 0
    long long mat_off;          // float index of the clade matrix entry [leaf_begin][leaf_begin]: of the maximal range around it
    int mat_n;                  // that matrix's side
    int node, leaf_begin, leaf_count, link_begin, link_count;
    int nb;                     // blocks per row
    int pad;
};

struct HommolaBlock {
    int64_t clade, p, row;      // row = clade * (permutations + 1) + p
    int64_t first, len;         // pairs [first, first + len) of the row
};

struct HommolaChunk {
    int64_t block_begin, n_blocks;      // global blocks [block_begin, block_begin + n_blocks)
    int64_t row_begin, n_rows;          // the rows they belong to
    int64_t rel_begin, n_rel;           // the relabelled positions of those rows
    unsigned side0_classes;             // bit k: a clade-side sort of size class k is needed (PermSortClass)
};

struct HommolaRange {
    int32_t leaf_begin, leaf_count;
    int64_t mat_off;                    // float index of the range's matrix
};

struct HommolaPlan {
    int64_t n_clades = 0, rows_per_clade = 0, n_rows = 0, n_blocks = 0, n_rel = 0;
    int32_t n_univ_o = 0, n_univ_c = 0;
    std::vector<HommolaCladeDev> clades;      // n_clades + 1
    std::vector<HommolaRange> ranges;         // the maximal ranges, by leaf_begin
    int64_t mat_floats = 0;                   // n_univ_o^2 + sum of the ranges' squares
    std::vector<HommolaChunk> chunks;
    int64_t max_chunk_blocks = 0, max_chunk_rel = 0;

    int64_t clade_of_block(int64_t t) const;      // the clade whose rows hold global block t
    HommolaBlock block(int64_t t) const;
    int64_t row_rel(int64_t row) const;           // global index of the row's first relabelled position
};

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: the sizes (universes within the limit, nothing negative), the
// positions (inside their universe; pos_c non-decreasing), every clade (its leaf range inside the universe, its link
// range exactly the links inside the leaf range), the clade ranges (laminar: nested or disjoint).  Then the layout
// above and the cut into chunks: chunk_blocks 0 = chunks of up to kRowsChunkBlocks blocks and about kCladeChunkPairs pairs.
int hommola_plan(int32_t n_univ_o, int32_t n_univ_c, const int32_t *pos_o, const int32_t *pos_c, int64_t n_links,
                 const st_hommola_clade *clades, int64_t n_clades, int64_t permutations, int64_t chunk_blocks, HommolaPlan &P,
                 std::string &err);

// pieces[n] of global blocks [block_begin, block_begin + n) into out[row] (n_rows entries, moments_empty() before the
// first block of a row): clade_merge in block order
void hommola_fold(const HommolaPlan &P, int64_t block_begin, int64_t n, const CladePiece *pieces, st_pair_moments *out);

}  // namespace st
