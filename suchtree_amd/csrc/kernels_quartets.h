// kernels_quartets.h -- part of suchtree_hip.hip: the device side of the quartet comparison
// (st_compare_quartets_*_host, st_quartet_positions; driver: host_quartets.h).
//
//   k_quartet_draw<MODE>  one lane per quartet: unranks (ST_QUARTET_ALL) or draws (ST_QUARTET_SAMPLE) its four positions
//                         (quartet_plan.h, the same inline functions as the host restatement) and writes ids_x[p] and
//                         ids_y[p] as two C-order int64 (c,4) rows -- what SrcQuartet reads -- or, for
//                         st_quartet_positions, the positions themselves.  16-byte stores.
//   k_quartet_agree       one lane per quartet: the six MRCA ids of the quartet in tree X and in tree Y (written by the
//                         MRCA kernels over SrcQuartet), the class of each (quartet_class), cell = 4 class_x + class_y.
//                         A wave counts each cell with a ballot and a population count -- the sixteen running counts
//                         are wave-uniform --, the workgroup's waves meet in sixteen LDS counters and one lane per
//                         cell adds them to the global table: integer atomics only, so the table does not depend on
//                         grid, chunk or order.
#pragma once
#include "quartet_plan.h"

namespace st {

constexpr int kQuartetBlocks = 1024;
constexpr int kQuartetThreads = 256;

struct QuartetMulHiDevice {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return __umul64hi(a, b); }
};

// out_x / out_y: (n,4) int64 rows of ids (both or neither); out_pos: (n,4) int32 positions (or NULL)
template <int MODE>
__global__ __launch_bounds__(kQuartetThreads) void k_quartet_draw(const long long *__restrict__ ids_x, const long long *__restrict__ ids_y,
                                                                  unsigned long long seed, long long m, long long k0, long long n,
                                                                  long long *__restrict__ out_x, long long *__restrict__ out_y,
                                                                  int *__restrict__ out_pos)
{
    const long long stride = (long long)gridDim.x * kQuartetThreads;
    for (long long i = (long long)blockIdx.x * kQuartetThreads + threadIdx.x; i < n; i += stride) {
        int32_t p[4];
        quartet_positions_of<MODE>(seed, (uint64_t)(k0 + i), m, p, QuartetMulHiDevice{});
        if (out_pos) reinterpret_cast<int4 *>(out_pos)[i] = make_int4(p[0], p[1], p[2], p[3]);
        if (out_x) {
            longlong2 *ox = reinterpret_cast<longlong2 *>(out_x) + 2 * i, *oy = reinterpret_cast<longlong2 *>(out_y) + 2 * i;
            ox[0] = make_longlong2(ids_x[p[0]], ids_x[p[1]]);
            ox[1] = make_longlong2(ids_x[p[2]], ids_x[p[3]]);
            oy[0] = make_longlong2(ids_y[p[0]], ids_y[p[1]]);
            oy[1] = make_longlong2(ids_y[p[2]], ids_y[p[3]]);
        }
    }
}

// the six ids of quartet i: three 8-byte loads (24 i is a multiple of 8)
__device__ __forceinline__ int quartet_class_at(const int *__restrict__ M, long long i)
{
    const int2 *q = reinterpret_cast<const int2 *>(M) + 3 * i;
    const int2 a = q[0], b = q[1], c = q[2];
    const int32_t m[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
    return quartet_class(m);
}

// Mx / My: 6 n MRCA ids each; table: the 16 cells of st_quartet_table.cell, added to
__global__ __launch_bounds__(kQuartetThreads) void k_quartet_agree(const int *__restrict__ Mx, const int *__restrict__ My, long long n,
                                                                   unsigned long long *__restrict__ table)
{
    __shared__ unsigned cells[16];
    if (threadIdx.x < 16) cells[threadIdx.x] = 0u;
    __syncthreads();
    unsigned count[16];
#pragma unroll
    for (int c = 0; c < 16; c++) count[c] = 0u;
    const long long stride = (long long)gridDim.x * kQuartetThreads;
    const int lane = threadIdx.x & 63;
    // (base is the wave's first quartet: the trip count is wave-uniform, lanes past n vote for no cell)
    for (long long base = (long long)blockIdx.x * kQuartetThreads + (threadIdx.x - lane); base < n; base += stride) {
        const long long i = base + lane;
        const int cell = i < n ? 4 * quartet_class_at(Mx, i) + quartet_class_at(My, i) : -1;
#pragma unroll
        for (int c = 0; c < 16; c++) count[c] += (unsigned)__popcll(__ballot(cell == c));
    }
    // (a workgroup sees fewer than 2^31 / 6 quartets per launch: no counter overflows)
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 16; c++)
            if (count[c]) atomicAdd(&cells[c], count[c]);
    }
    __syncthreads();
    if (threadIdx.x < 16 && cells[threadIdx.x]) atomicAdd(&table[threadIdx.x], (unsigned long long)cells[threadIdx.x]);
}

}  // namespace st
