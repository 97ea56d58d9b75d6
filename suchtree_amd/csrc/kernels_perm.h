// kernels_perm.h -- included by suchtree_hip.hip (before kernels_hommola.h and kernels_dispersion.h, which sort with it).
// The device sort of the keyed permutation (keyed_perm.h): the keys w_i of a universe sorted, sigma[j] = low 16 bits of
// the j-th smallest.  Up to 64 positions: one wave, keys in registers, a bitonic network of lane exchanges; larger ones:
// one workgroup, keys in perm_lds_bytes(n) of LDS.  And st_hommola_permutation's kernels: one such sort.
//
// The LDS sort: stages whose partner distance j is 64 or more exchange through LDS -- consecutive lanes read
// consecutive 8-byte keys, so a 32-lane group covers one 256-byte bank row without a conflict; stages with j <= 32 would
// read 8-byte keys 16 .. 512 bytes apart (2- to 32-way conflicts), so each lane takes one key into a register instead and
// the wave runs those stages as lane exchanges, as the one-wave form does.
//
#pragma once

#include "keyed_perm.h"

namespace st {

// stages j0, j0 / 2, ... 1 (j0 <= 32) of merge level k of a bitonic sort, on the key of element i held by lane i % 64
__device__ __forceinline__ unsigned long long perm_lane_stages(unsigned long long v, unsigned i, unsigned k, unsigned j0)
{
    for (unsigned j = j0; j > 0; j >>= 1) {
        const unsigned long long o = __shfl_xor(v, (int)j);
        const bool up = (i & k) == 0, lower = (i & j) == 0;
        v = (lower == up) ? (v < o ? v : o) : (v < o ? o : v);
    }
    return v;
}

// the keys of h1 over n positions sorted in LDS (keys: room for n rounded up to a power of two, at least 128); every
// lane of the workgroup of T calls it, and a barrier closes it
template <int T>
__device__ __forceinline__ void perm_sort_lds(unsigned long long *keys, unsigned long long h1, unsigned n, unsigned tid)
{
    unsigned N = 128;      // a power of two, whole waves
    while (N < n) N <<= 1;
    for (unsigned i = tid; i < N; i += T) keys[i] = i < n ? perm_key(h1, i) : ~0ull;
    __syncthreads();
    for (unsigned k = 2; k <= N; k <<= 1) {
        for (unsigned j = k >> 1; j >= 64; j >>= 1) {
            for (unsigned q = tid; q < N / 2; q += T) {
                const unsigned lo = 2 * q - (q & (j - 1)), hi = lo + j;
                const unsigned long long u = keys[lo], v = keys[hi];
                if ((u > v) == ((lo & k) == 0)) {
                    keys[lo] = v;
                    keys[hi] = u;
                }
            }
            __syncthreads();
        }
        for (unsigned i = tid; i < N; i += T) keys[i] = perm_lane_stages(keys[i], i, k, k >> 1 < 32 ? k >> 1 : 32);
        __syncthreads();
    }
}

// the same for up to 64 positions: lane i's key in, the i-th smallest out
__device__ __forceinline__ unsigned long long perm_sort_wave(unsigned long long h1, int n, int lane)
{
    unsigned long long key = lane < n ? perm_key(h1, (unsigned)lane) : ~0ull;
    for (unsigned k = 2; k <= 64; k <<= 1) key = perm_lane_stages(key, (unsigned)lane, k, k >> 1);
    return key;
}

// st_hommola_permutation on the device: one sort of n positions by the form its size class takes, sigma as int32
template <int T>
__global__ __launch_bounds__(T) void k_hommola_permutation(unsigned long long seed, int node, long long p, int side, int n, int *out)
{
    extern __shared__ unsigned long long perm_keys[];
    const unsigned tid = threadIdx.x;
    if (p != 0) perm_sort_lds<T>(perm_keys, perm_stream(seed, node, p, side), (unsigned)n, tid);
    for (unsigned i = tid; i < (unsigned)n; i += T) out[i] = p == 0 ? (int)i : (int)(perm_keys[i] & 0xFFFF);
}

__global__ __launch_bounds__(64) void k_hommola_permutation_wave(unsigned long long seed, int node, long long p, int side, int n, int *out)
{
    const int lane = threadIdx.x;
    const unsigned long long key = p != 0 ? perm_sort_wave(perm_stream(seed, node, p, side), n, lane) : (unsigned long long)lane;
    if (lane < n) out[lane] = (int)(key & 0xFFFF);
}

}  // namespace st
