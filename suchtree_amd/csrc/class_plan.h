// class_plan.h -- the host-only side of the per-class sums of a distance matrix under relabelling (st_class_sums_codes:
// compare.mantel_correlogram), plain C++17.  No GPU calls in here (class_plan.cpp): the "not gpu" tests run it under the
// address / undefined-behaviour sanitizers (tests/emu/sanitize_class.cpp).  The definitions are the contract of
// include/suchtree_hip.h (st_class_sums_codes); the permutation, its blocks and the chunk record are those of
// dispersion_plan.h, the cut into tasks that of its SlicedPlan.
//
// Layout.  n > kClassWaveMax: the row form.  An item is a row pair r < (n + 1) / 2 -- rows r and n - 1 - r, the middle
// row alone when n is odd -- so that every item has n - 1 pairs (the middle row half as many).  A block of n_perms
// permutations from p0 is cut into n_slices = ceil(n_perms / slice) slices of `slice` permutations (the last one shorter);
// task t = r * n_slices + s is row pair r under slice s, whose workgroup stages its rows of y once for all the slice's
// permutations and leaves n_classes partial sums per (row pair, permutation).  Up to kClassWaveMax: the wave form, one
// item, task t is permutation p0 + t of the block.  A chunk is a range of t of one block.
#pragma once
#include "dispersion_plan.h"
#include "plan_checks.h"

namespace st {

constexpr int kClassMax = ST_CLASS_MAX;                   // classes per call: one lane each when a wave reads its accumulators
constexpr int kClassNone = ST_CLASS_NONE;                 // the byte of a pair in no class (and of the square's diagonal and padding)
constexpr int kClassWaveMax = 64;                         // matrices of up to 64 rows: row l in lane l, y and the class square in LDS
constexpr int kClassWaveStride = kClassWaveMax + 1;       // the wave form's LDS row stride of y in words: odd, as kGroupWaveStride
constexpr int kClassWaveBytes = kClassWaveMax + 4;        // the wave form's LDS row stride of the class square in bytes: 17 words, odd
constexpr int kClassThreads = 256;                        // the workgroup of every kernel
constexpr int kClassCopies = 4;                           // accumulators per class and wave, by lane & 3: a row in one class meets 16 lanes an address, not 64
constexpr int kClassSlice = 32;                           // permutations per task of the row form: DESIGN.md section 26 has the sweep
constexpr int kClassSliceMax = 256;                       // bound of SUCHTREE_AMD_CLASS_SLICE
constexpr int64_t kClassPartBytes = (int64_t)256 << 20;   // bound of a block's partial sums (8 n_classes bytes per row pair and permutation)

struct ClassPlan : SlicedPlan {      // rows of out; a row of the class square is sliced_stride(n) bytes
    int32_t n_classes = 0;
};

// pair (a, b), a != b, of the triangle
inline size_t class_pair(int32_t a, int32_t b) { return a > b ? (size_t)a * (size_t)(a - 1) / 2 + (size_t)b : (size_t)b * (size_t)(b - 1) / 2 + (size_t)a; }

// ST_OK, or ST_ERR_ARG with `err`.  Checks, in this order: those of dispersion_call_args (n in 3 .. kPermMaxUniverse,
// nothing negative among permutations, chunk_tasks, stream), at most 2^31 - 1 permutations, n_classes in 1 .. kClassMax,
// NULL pointers (y, cls, out), then the first cls[k] that is neither below n_classes nor kClassNone.  Then the layout
// above for `slice` in 1 .. kClassSliceMax: chunk_tasks 0 = blocks of up to kDispersionSigmaBytes of sigma rows and
// kClassPartBytes of partial sums, chunks of kDispersionChunkTasks tasks; chunk_tasks > 0 = at most that many tasks per
// chunk and permutations per block.
int class_plan(const int32_t *y, const uint8_t *cls, int32_t n, int32_t n_classes, int64_t permutations, int32_t stream, int64_t chunk_tasks,
               int32_t slice, const int64_t *out, ClassPlan &P, std::string &err);

// what row i adds under sigma: acc[c] += y_row[j] over j < i, c = cls[pair (sigma[i], sigma[j])], where c is a class
void class_row(const int32_t *y_row, const uint8_t *cls, const int32_t *sigma, int32_t i, int64_t *acc);

// every row of the call on the host: out[p * n_classes + c], the rows and the fold of the kernels
void class_host(const int32_t *y, const uint8_t *cls, const ClassPlan &P, uint64_t seed, int32_t stream, int64_t *out);

}  // namespace st
