// mantel_plan.h -- the host-only side of the Mantel and partial Mantel sums (st_mantel_codes, st_mantel_quantise), plain
// C++17.  No GPU calls in here (mantel_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour
// sanitizers (tests/emu/sanitize_mantel.cpp).  The definitions are the contract of include/suchtree_hip.h
// (st_mantel_codes); the permutation, its blocks and the chunk record are those of dispersion_plan.h.
//
// Layout.  n <= kMantelWaveMax: the wave form, one item, a task is a permutation.  Above: the row form, an item is a row
// pair r < (n + 1) / 2 -- rows r and n - 1 - r, the middle row alone when n is odd -- so that every item has about n
// pairs.  Within a block of n_perms permutations from p0, task t = r * n_perms + (p - p0), as in DispersionPlan; a chunk
// is a range of t of one block.
#pragma once
#include "dispersion_plan.h"
#include "plan_checks.h"

namespace st {

constexpr int kMantelWaveMax = 64;                        // matrices of up to 64 rows: row l in lane l, x_sq in LDS
constexpr int kMantelThreads = 256;                       // the workgroup of both forms
constexpr int kMantelWaveStride = kMantelWaveMax + 1;     // the wave form's LDS row stride in words: odd, so the 64 rows of a column lie in 64 banks
constexpr int64_t kMantelBlockTasks = (int64_t)1 << 22;   // bound of a block's partial records (32 bytes each)
constexpr int32_t kMantelShiftLimit = 2000;               // |shift| of a caller's shift

using i128 = __int128;

struct MantelPlan : MatrixPlan {      // items: 1 (wave form) or (n + 1) / 2 row pairs
    int32_t n = 0;
    bool partial = false;
};

inline st_mantel_sums mantel_sums(i128 xy, i128 xz)
{
    return st_mantel_sums{(uint64_t)xy, (int64_t)(xy >> 64), (uint64_t)xz, (int64_t)(xz >> 64)};
}

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: those of dispersion_call_args (n in 3 .. kPermMaxUniverse,
// nothing negative among permutations, chunk_tasks, stream), at most 2^31 - 1 permutations, NULL pointers (x_sq, y,
// moments, out; z may be NULL: the simple test), then the symmetry of x_sq, naming the first cell (row-major) whose
// mirror differs.  Then the layout above and the invariant sums over the pairs j < i, x taken from the lower triangle,
// in __int128: chunk_tasks 0 = blocks of up to kDispersionSigmaBytes of sigma rows and kMantelBlockTasks tasks, chunks
// of kDispersionChunkTasks tasks; chunk_tasks > 0 = at most that many tasks per chunk and permutations per block.
int mantel_plan(const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, int64_t permutations, int32_t stream, int64_t chunk_tasks,
                st_mantel_moments *moments, const st_mantel_sums *out, MantelPlan &P, std::string &err);

// the sums of x relabelled by sigma[0 .. n) against y and, where z is not NULL, z
void mantel_record(const int32_t *x_sq, const int32_t *y, const int32_t *z, int32_t n, const int32_t *sigma, i128 &sxy, i128 &sxz);

// every record of the call on the host: out[p]
void mantel_host(const int32_t *x_sq, const int32_t *y, const int32_t *z, const MantelPlan &P, uint64_t seed, int32_t stream, st_mantel_sums *out);

// q(v) = llrint(ldexp(v, shift)) as int32 (the contract's fixed point): ST_OK, or ST_ERR_ARG with `err`
int mantel_quantise(const double *v, int64_t n, int32_t shift, int32_t *out, int32_t *out_shift, std::string &err);

}  // namespace st
