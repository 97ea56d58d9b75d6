// parafit_plan.h -- the host-only side of ParaFit's global and link statistics (st_parafit_codes), plain C++17.  No GPU
// calls in here (parafit_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour sanitizers
// (tests/emu/sanitize_parafit.cpp).  The definitions are the contract of include/suchtree_hip.h (st_parafit_codes); the
// permutation is keyed_perm.h's, the chunk record and the cut into blocks and chunks dispersion_plan.h's.
//
// Layout.  The links are sorted by (f, s), so the links of one F position are one range; `groups` lists the F positions
// that have links.  Within a block of n_perms permutations from p0 the relabelled S positions are R[(p - p0) * L + l] and
// the record of link l under permutation p is part[l * n_perms + (p - p0)].  Wave form (L <= 64 and n_s <= 64): one item,
// a task is a permutation.  Row form: L items, task t = l * n_perms + (p - p0), a chunk is a range of t of one block.
#pragma once
#include "dispersion_plan.h"
#include "mantel_plan.h"
#include "plan_checks.h"

namespace st {

constexpr int kParafitWaveMax = 64;                         // up to 64 links over up to 64 S positions: link l in lane l
constexpr int kParafitThreads = 256;                        // the workgroup of both forms
constexpr int kParafitWaveStride = kParafitWaveMax + 1;     // the wave form's LDS row stride in words (odd: 64 rows of a column in 64 banks)
constexpr int64_t kParafitBlockTasks = (int64_t)1 << 22;    // bound of a block's link records (32 bytes each)

// the record of one link under one permutation: Link1 = 2 x row sum - diagonal term, and the row sum
struct ParafitRecord {
    uint64_t link_lo;
    int64_t link_hi;
    uint64_t row_lo;
    int64_t row_hi;
};

struct ParafitGroup {
    int32_t f, stream;             // the F position and its stream id
    int32_t begin, count;          // its links [begin, begin + count)
};

struct ParafitPlan : MatrixPlan {      // items: 1 (wave form) or L
    int32_t n_f = 0, n_s = 0, n_links = 0;
    std::vector<ParafitGroup> groups;     // the F positions with links, ascending
};

inline st_parafit_sum parafit_sum(i128 v) { return st_parafit_sum{(uint64_t)v, (int64_t)(v >> 64)}; }
inline i128 parafit_i128(uint64_t lo, int64_t hi) { return (i128)(((unsigned __int128)(uint64_t)hi << 64) | lo); }

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: n_f, n_s and n_links each in 3 .. kPermMaxUniverse; nothing
// negative among permutations and chunk_tasks; at most 2^31 - 1 permutations; NULL inputs (g_f, g_s, link_f, link_s,
// stream_f); NULL outputs (total, link_obs, link_n_ge; link_all may be NULL); link by link a position outside its
// universe, then a link that is not above the one before in (f, s) order (unsorted or repeated), each naming the link;
// a negative stream_f[i], naming i; the symmetry of g_f, then of g_s, naming the first cell (row-major) whose mirror
// differs.  Then the layout above: chunk_tasks 0 = blocks of up to kDispersionSigmaBytes of R and kParafitBlockTasks
// records, chunks of kDispersionChunkTasks tasks; chunk_tasks > 0 = at most that many tasks per chunk and permutations
// per block.
int parafit_plan(const int32_t *g_f, int32_t n_f, const int32_t *g_s, int32_t n_s, const int32_t *link_f, const int32_t *link_s, int32_t n_links,
                 const int32_t *stream_f, int64_t permutations, int64_t chunk_tasks, const st_parafit_sum *total, const st_parafit_sum *link_obs,
                 const int64_t *link_n_ge, ParafitPlan &P, std::string &err);

// r[0 .. L): the S position of every link under permutation p (p = 0: link_s itself)
void parafit_relabel(const ParafitPlan &P, const int32_t *link_s, uint64_t seed, int64_t p, int32_t *r);

// the records of the links relabelled to r[0 .. L), and their total (the sum of the row sums)
void parafit_records(const int32_t *g_f, const int32_t *g_s, const ParafitPlan &P, const int32_t *link_f, const int32_t *r, ParafitRecord *rec, i128 &total);

// the whole call on the host
void parafit_host(const int32_t *g_f, const int32_t *g_s, const ParafitPlan &P, const int32_t *link_f, const int32_t *link_s, uint64_t seed,
                  st_parafit_sum *total, st_parafit_sum *link_obs, int64_t *link_n_ge, st_parafit_sum *link_all);

}  // namespace st
