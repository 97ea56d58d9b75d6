// clade_match_plan.h -- the host-only side of the clade matching behind Robinson-Foulds and transfer support
// (st_clade_ranges, st_clade_match), plain C++17, and what the device shares with it (kernels_clade_match.h): the
// limits, the distance of a pair of ranges and the packed key.  No GPU calls in here (clade_match_plan.cpp): the
// "not gpu" tests run it under the address / undefined-behaviour sanitizers (tests/emu/sanitize_clade_match.cpp).  The
// definitions are the contract of include/suchtree_hip.h (st_clade_match).
//
// Layout.  A row is a range [lo, hi) of tree A's leaf positions, a candidate a range of tree B's; pos_b takes an A
// position to the B position of the same leaf.  The device form sorts the candidates by size (stable, so equal sizes
// keep B's order) and gives every row up to two windows of that sorted list: the candidates whose size alone does not
// rule out a distance below p - 1.  Rows are cut into chunks of up to `chunk` rows, one launch and one read-back each.
// Everything is an int32 or the uint64 key: nothing depends on the order of a reduction, on the windows or on the cut.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "quartet_plan.h"      // ST_QUARTET_HD, the public header

namespace st {

constexpr int32_t kCladeMatchMinLeaves = 4;
constexpr int32_t kCladeMatchMaxLeaves = ST_CLADE_MATCH_MAX_LEAVES;
constexpr int kCladeMatchThreads = 256;                       // the workgroup of k_clade_match: four waves
constexpr int kCladeMatchBlocks = 4096;                       // the grid's cap: a workgroup strides over a chunk's rows
constexpr int64_t kCladeMatchChunkRows = 65536;               // default rows per chunk
constexpr uint64_t kCladeMatchNoKey = ~(uint64_t)0;           // the key of "no candidate"

// 64-bit words of the bitmap of m positions: one of padding, so rank(m) reads a word when m is a multiple of 64
ST_QUARTET_HD int32_t clade_match_words(int32_t m) { return (m >> 6) + 1; }

// LDS of a workgroup: the bitmap words, one uint32 running count per word, then (16-byte aligned) 64 bytes in which the
// waves meet: 48 KiB + 76 bytes at the cap
ST_QUARTET_HD size_t clade_match_lds_tail(int32_t m) { return ((size_t)clade_match_words(m) * 12 + 15) & ~(size_t)15; }
ST_QUARTET_HD size_t clade_match_lds_bytes(int32_t m) { return clade_match_lds_tail(m) + 64; }

// delta of a row of size sa and a candidate of size sb that share i leaves, among m
ST_QUARTET_HD int32_t clade_match_delta(int32_t sa, int32_t sb, int32_t i, int32_t m, bool unrooted)
{
    const int32_t d = sa + sb - 2 * i;
    return unrooted && m - d < d ? m - d : d;
}

ST_QUARTET_HD uint64_t clade_match_key(int32_t delta, int32_t index) { return ((uint64_t)(uint32_t)delta << 32) | (uint32_t)index; }

// p - 1: what a row's transfer distance cannot exceed
ST_QUARTET_HD int32_t clade_match_bound(int32_t sa, int32_t m, bool unrooted) { return (unrooted && m - sa < sa ? m - sa : sa) - 1; }

// The order and the eligible induced clades of one tree (st_clade_ranges).  ST_OK, ST_ERR_ARG / ST_ERR_TREE with `err`,
// or ST_ERR_BOUNDS; *bad_id (may be NULL) names the id behind ST_ERR_BOUNDS and behind an id that is no leaf or repeated.
// order has m entries on return, node / lo / hi one per eligible clade, in breadth-first order of the nodes.
int clade_ranges(const int32_t *parent, int64_t n_nodes, const int64_t *leaf_ids, int32_t m, bool rooted, std::vector<int32_t> &order,
                 std::vector<int32_t> &node, std::vector<int32_t> &lo, std::vector<int32_t> &hi, int64_t *bad_id, std::string &err);

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: m in range, no negative count or chunk, NULL arrays, pos_b a
// permutation of 0 .. m - 1, A's ranges then B's inside [0, m] with lo < hi.
int clade_match_args(int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo,
                     const int32_t *b_hi, int32_t n_b, int64_t chunk_rows, std::string &err);

// the restatement of the definition: every row against every candidate in B's order, through one prefix count per row
void clade_match_host(int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo,
                      const int32_t *b_hi, int32_t n_b, bool unrooted, int32_t *out_distance, int32_t *out_match, int32_t *out_intersection);

struct CladeMatchPlan {
    int32_t m = 0, n_a = 0, n_b = 0;
    bool unrooted = false;
    int64_t chunk = 0;                          // rows per chunk, >= 1
    std::vector<int32_t> b_lo, b_hi, b_idx;     // the candidates by size (stable); b_idx = the index in B's list
    std::vector<int32_t> win;                   // 4 per row: sorted candidates [w0, w1) and [w2, w3), disjoint; all 0 = none
};

// the sorted candidates and the rows' windows (use_window false: no windows, every row scans all candidates)
void clade_match_plan(int32_t m, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo, const int32_t *b_hi, int32_t n_b,
                      bool unrooted, int64_t chunk_rows, bool use_window, CladeMatchPlan &P);

// what the kernel computes, on the host: the windows first, all candidates where they hold nothing below p - 1
void clade_match_windowed_host(const CladeMatchPlan &P, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t *out_distance,
                               int32_t *out_match, int32_t *out_intersection);

}  // namespace st
