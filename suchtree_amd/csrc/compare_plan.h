// compare_plan.h -- the host-only side of the compare paths (st_compare_*_host, st_clade_plan), plain C++17: the
// plain structs the device and the host share, the checks of caller-supplied arrays, the clade plan and its tables,
// the rows layout, and the folding of pieces into records.  No GPU calls in here (compare_plan.cpp): the "not gpu"
// tests run this file under the address / undefined-behaviour sanitizers (tests/emu/sanitize_main.cpp).
// Errors: a code (ST_OK / ST_ERR_*) and the message in `err`.  Ids out of range have no message here: the caller words
// them with report_fault (host_launch.h), from the extremes ids_in_range leaves.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/suchtree_hip.h"

namespace st {

// ---- shared with the device (device_common.h: SrcSegments; kernels_clades.h, kernels_rows.h) ----------------------
constexpr int kCladeTileShift = 13;      // 8192 pairs per tile (ST_CLADE_TILE)
static_assert((1 << kCladeTileShift) == ST_CLADE_TILE, "kCladeTileShift");
struct CladeSeg {
    long long first;       // k of the segment's first pair
    int r0, r1;            // row positions [r0, r1)
    int c0, c1;            // column positions [c0, c1); c0 < 0: the triangle over [r0, r1)
};
struct CladeTile {
    int seg;               // the segment of the tile's first pair (the sentinel's index past the last tile)
    int piece;             // index of the tile's first piece (kernels_clades.h)
};
struct CladePiece {
    double sx, sy, sxx, syy, sxy;          // sums of (x - cx), (y - cy), squares and cross product
    float cx, cy;                          // the shift: the piece's first pair (0 where that is not finite)
    float min_x, max_x, min_y, max_y;      // NaN-ignoring; +inf / -inf when nothing was seen
};

constexpr int64_t kCladeChunkPairs = (int64_t)1 << 25;      // 2 x 128 MiB of float32 distances, as the triangle
constexpr int64_t kRowsChunkBlocks = (int64_t)1 << 18;      // 16 MiB of pieces per buffer

// ---- moments -------------------------------------------------------------------------------------------------------
st_pair_moments moments_empty();        // n = 0, zero sums, NaN min / max: fewer than two links, no pairs
st_pair_moments piece_moments(const CladePiece &c, int64_t n);      // a piece of n pairs, about its own shift
// Chan's pairwise update on shifted sums, in the operation order of compare.DistanceComparison.merge: b moved to a's shift
void clade_merge(st_pair_moments &a, const st_pair_moments &b);

// ---- checks of what the caller supplies -----------------------------------------------------------------------------
// all NULL (no histogram), or bins >= 1, at most max_cells cells, finite increasing edges
int compare_hist_args(const double *edges_x, int32_t bins_x, const double *edges_y, int32_t bins_y, const int64_t *out_hist,
                      int64_t max_cells, std::string &err);
// false when an id lies outside [0, n_nodes): max_bad / min_bad (a Fault's words, initialised by the caller) then hold
// the extremes of the offending ids
bool ids_in_range(const int64_t *ids, int64_t n, int64_t n_nodes, long long &max_bad, long long &min_bad);

// ---- every clade at once ------------------------------------------------------------------------------------------
// The clade tree's children in increasing id order, its preorder, the permutation that makes every clade one range of
// link positions, and the segments.  Iterative throughout (a caterpillar of 1e5 levels is fine).
struct CladePlan {
    std::vector<int64_t> child_off, child;       // CSR: children of v are child[child_off[v] .. child_off[v + 1])
    std::vector<int64_t> pre;                    // preorder (children in order); reversed, every child precedes its parent
    std::vector<int64_t> perm, begin, count, leaves;
    std::vector<st_clade_segment> segs;          // in pair order: nodes by link count, each node's own segments together
    std::vector<int64_t> node_seg;               // node v's segments: segs[node_seg[v] .. node_seg[v] + node_nseg[v])
    std::vector<int32_t> node_nseg;
    int64_t total = 0;
};
// Errors in this order: the tree's structure (ST_ERR_TREE), link ids out of range (ST_ERR_BOUNDS, no message), a link
// on an inner node (ST_ERR_ARG).  cap < 0: no cap.
int clade_plan(const int32_t *parent, int64_t n, const int64_t *link_leaf, int64_t L, int64_t cap, CladePlan &P,
               std::string &err);

// What the device reads of a plan.  tile[t].seg = the segment of pair t * TILE, tile[t].piece = pieces before tile t; a
// sentinel segment (first = total) and a sentinel tile close the tables.
struct CladeTables {
    std::vector<CladeSeg> segs;
    std::vector<CladeTile> tiles;
    std::vector<int64_t> seg_piece;       // segment s's pieces: [seg_piece[s], seg_piece[s + 1])
    int64_t n_pieces = 0;
};
bool clade_tables(const CladePlan &P, CladeTables &T);      // false: more than 2^31 - 1 pieces (indices are int32)
// pieces[T.n_pieces] -> out[n_nodes]: pieces into segments (index order), segments into nodes (children first, in id
// order, then the node's own segments); a node over the cap is not computed: n = -1, NaN elsewhere
void clade_fold(const CladePlan &P, const CladeTables &T, const CladePiece *pieces, int64_t cap, st_pair_moments *out);

// ---- many triangles at once (st_compare_rows_host) ----------------------------------------------------------------
// Row r's pairs sit at global index r * S + k (SrcRows).  Rows of at most half a chunk are dense (S = P; a chunk holds
// whole rows, at most kRowsChunkBlocks blocks' worth so that tiny rows do not make huge piece buffers); larger rows are
// padded to whole tiles (S = P rounded up) and a chunk is whole tiles.  Either way no block straddles a chunk.
struct RowsLayout {
    int64_t P = 0, S = 0, nb = 0, chunk = 0, max_rows = 0, max_blocks = 0;

    int64_t block_of(int64_t g) const;       // the block of global pair g (padding: its row's last block)
    int64_t block_lo(int64_t t) const;       // global index of block t's first pair
    int64_t block_len(int64_t t) const;      // its pairs
};
RowsLayout rows_layout(int64_t n_rows, int64_t m, int64_t chunk_pairs);      // chunk_pairs 0: kCladeChunkPairs

}  // namespace st
