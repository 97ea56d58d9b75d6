// kernels_dispersion.h -- included by suchtree_hip.hip (after kernels_perm.h, whose sorts it uses).
// The device side of st_partner_dispersion_host and st_dispersion_matrix (layout and order rule: dispersion_plan.h; the
// contract: include/suchtree_hip.h).  Task (set, p) relabels the set's positions through sigma_p and reduces the k x k
// sub-matrix D[q_i][q_j] of the float32 matrix D: every row's sum over j != i and its minimum, then both over i.
//
//   k_dispersion_sigma   one sort per permutation p of the chunk's block (not per task): the keys of perm_stream(seed,
//                        stream, p, 0) over the universe, sorted by perm_sort_wave / perm_sort_lds, the low 16 bits
//                        as one uint16 row of sigma.  p = 0 writes the identity.
//   k_dispersion_tasks   three forms, one per size class; element i of a task is a lane's, the lane walks j:
//       packed     K' <= 32: 64 / K' tasks per wave, q_j from lane j of the task's K'-lane group, the butterfly inside it;
//       wave       33 <= k <= 64: one task per wave, q_j read from lane j at a wave-uniform j (a scalar);
//       workgroup  k > 64: 256 lanes, q staged in LDS as uint16 (up to 32 KiB), eight q_j per 16-byte broadcast read;
//                  lane t takes the elements t, t + 256, ...
//     In every form a step of the j loop issues kDispersionUnroll independent 4-byte gathers D[q_i * N + q_j] before
//     the first add (the row q_i is up to 64 KiB: a gather is an L2 or Infinity Cache hit whose latency only other
//     loads in flight hide), then adds them in j order.  The j == i entry is loaded and left out of both results.
//
//     Each form is instantiated twice: k_dispersion_tasks_* read q_i = sigma_p[set_pos[begin + i]] (the taxa-labels null),
//     k_swap_tasks_* read q_i = table_p[begin + i] from the table rows that k_swap_chains writes (the swap null,
//     kernels_swap.h); everything after q_i is the same code.
//
// Determinism: a row's sum runs over j ascending in one lane; the order over i is that of dispersion_record
// (dispersion_plan.cpp), operation for operation.  No float atomics.
#pragma once

#include "dispersion_plan.h"

namespace st {

constexpr int kDispersionUnroll = 8;

struct DispersionSigmaArgs {
    unsigned short *sigma;      // row p - p0 of the block: n entries
    long long p0;
    unsigned long long seed;
    int stream, n;
};

template <int T>
__global__ __launch_bounds__(T) void k_dispersion_sigma(DispersionSigmaArgs a)
{
    extern __shared__ unsigned long long perm_keys[];
    const unsigned tid = threadIdx.x;
    const long long p = a.p0 + blockIdx.x;
    unsigned short *row = a.sigma + (size_t)blockIdx.x * (size_t)a.n;
    if (p == 0) {
        for (unsigned i = tid; i < (unsigned)a.n; i += T) row[i] = (unsigned short)i;
        return;
    }
    const unsigned long long h1 = perm_stream(a.seed, a.stream, p, 0);
    if (a.n <= kPermWaveMax) {      // (workgroup-uniform: no barrier on this path)
        if (tid >= 64) return;
        const unsigned long long key = perm_sort_wave(h1, a.n, (int)tid);
        if ((int)tid < a.n) row[tid] = (unsigned short)(key & 0xFFFF);
        return;
    }
    perm_sort_lds<T>(perm_keys, h1, (unsigned)a.n, tid);
    for (unsigned i = tid; i < (unsigned)a.n; i += T) row[i] = (unsigned short)(perm_keys[i] & 0xFFFF);
}

struct DispersionTaskArgs {
    const float *D;
    const unsigned short *sigma;         // the block's rows
    const int *set_pos;
    const DispersionSetDev *sets;        // the live sets in plan order
    st_dispersion_record *out;           // this launch's records: entry `slot`
    long long set0, n;                   // this launch: n tasks (n < 2^31), the first one of set set0 ...
    unsigned perm0, n_perms;             // ... under row perm0 of the block's n_perms: task slot is (set0, perm0) + slot, row-fastest
    int n_univ, lanes;                   // packed form: K'
    int n_pos;                           // table form: the entries of a table row
};

// one row's walk: `qj(j)` gives q_j for 0 <= j < k (k >= 1), i the lane's own element; a lane that is not live adds nothing
template <typename Q>
__device__ __forceinline__ void dispersion_row(const float *__restrict__ row, int k, int i, bool live, Q qj, double &sum, float &m)
{
    sum = 0.0;
    m = __builtin_inff();
    for (int j0 = 0; j0 < k; j0 += kDispersionUnroll) {
        float v[kDispersionUnroll];
#pragma unroll
        for (int u = 0; u < kDispersionUnroll; u++) v[u] = row[qj(min(j0 + u, k - 1))];
#pragma unroll
        for (int u = 0; u < kDispersionUnroll; u++) {
            const int j = j0 + u;
            if (live && j < k && j != i) {
                sum += (double)v[u];
                m = v[u] < m ? v[u] : m;
            }
        }
    }
}

// The two forms of a task's positions.  Sigma form (kTable = false): `sigma` holds the block's sigma rows, q_i =
// sigma_p[set_pos[begin + i]].  Table form (kTable = true, the swap null: kernels_swap.h): `sigma` holds the block's table
// rows of n_pos entries, the randomised sets themselves with the offsets of the observed ones, q_i = table_p[begin + i].
template <bool kTable>
__device__ __forceinline__ void dispersion_task(const DispersionTaskArgs &a, long long slot, DispersionSetDev &s, const unsigned short *&sig)
{
    const unsigned u = a.perm0 + (unsigned)slot, c = u / a.n_perms;      // (32 bits: perm0 < n_perms < 2^25, slot < 2^31)
    s = a.sets[a.set0 + c];
    sig = a.sigma + (size_t)(u - c * a.n_perms) * (size_t)(kTable ? a.n_pos : a.n_univ);
}

template <bool kTable>
__device__ __forceinline__ int dispersion_position(const DispersionTaskArgs &a, const unsigned short *sig, int at)
{
    return kTable ? (int)sig[at] : (int)sig[a.set_pos[at]];
}

template <bool kTable>
__device__ __forceinline__ void dispersion_tasks_packed(const DispersionTaskArgs &a)
{
    const int lane = threadIdx.x & 63, kp = a.lanes, li = lane & (kp - 1);
    const long long wave = (long long)blockIdx.x * (kDispersionThreads / 64) + (threadIdx.x >> 6);
    const long long slot = wave * (64 / kp) + lane / kp;      // (the lanes of a group agree)
    const bool task = slot < a.n;
    DispersionSetDev s{0, 1};
    const unsigned short *sig = a.sigma;
    if (task) dispersion_task<kTable>(a, slot, s, sig);
    const bool live = task && li < s.count;
    const int q = live ? dispersion_position<kTable>(a, sig, s.begin + li) : 0;      // (an absent lane reads row 0, column 0, and adds nothing)
    // every group walks K' columns: the exchange needs all lanes of the wave, and q_j of an absent lane j is never added
    const int group = lane - li, k = s.count;
    double sum = 0.0;
    float m = __builtin_inff();
    const float *row = a.D + (size_t)q * (size_t)a.n_univ;
    for (int j0 = 0; j0 < kp; j0 += kDispersionUnroll) {
        float v[kDispersionUnroll];
#pragma unroll
        for (int u = 0; u < kDispersionUnroll; u++) v[u] = j0 + u < kp ? row[__shfl(q, group + j0 + u)] : 0.0f;      // (K' is wave-uniform)
#pragma unroll
        for (int u = 0; u < kDispersionUnroll; u++) {
            const int j = j0 + u;
            if (live && j < k && j != li) {
                sum += (double)v[u];
                m = v[u] < m ? v[u] : m;
            }
        }
    }
    double nearest = live ? (double)m : 0.0;
    for (int o = kp >> 1; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        nearest += __shfl_xor(nearest, o);
    }
    if (task && li == 0) a.out[slot] = st_dispersion_record{sum, nearest};
}

template <bool kTable>
__device__ __forceinline__ void dispersion_tasks_wave(const DispersionTaskArgs &a)
{
    const int lane = threadIdx.x & 63;
    const long long slot = (long long)blockIdx.x * (kDispersionThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.n) return;      // (wave-uniform; no workgroup barrier below)
    DispersionSetDev s;
    const unsigned short *sig;
    dispersion_task<kTable>(a, slot, s, sig);
    s = DispersionSetDev{__builtin_amdgcn_readfirstlane(s.begin), __builtin_amdgcn_readfirstlane(s.count)};      // (scalars: the j loop is uniform)
    const bool live = lane < s.count;
    const int q = live ? dispersion_position<kTable>(a, sig, s.begin + lane) : 0;
    double sum;
    float m;
    dispersion_row(a.D + (size_t)q * (size_t)a.n_univ, s.count, lane, live, [&](int j) { return __builtin_amdgcn_readlane(q, j); }, sum, m);
    double nearest = live ? (double)m : 0.0;
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        nearest += __shfl_xor(nearest, o);
    }
    if (lane == 0) a.out[slot] = st_dispersion_record{sum, nearest};
}

template <bool kTable>
__device__ __forceinline__ void dispersion_tasks_group(const DispersionTaskArgs &a)
{
    extern __shared__ uint4 dispersion_q[];      // q as uint16, eight to a 16-byte read, padded with position 0
    __shared__ double wave_sum[kDispersionThreads / 64], wave_near[kDispersionThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    DispersionSetDev s;
    const unsigned short *sig;
    dispersion_task<kTable>(a, blockIdx.x, s, sig);      // (workgroup-uniform)
    s = DispersionSetDev{__builtin_amdgcn_readfirstlane(s.begin), __builtin_amdgcn_readfirstlane(s.count)};
    unsigned short *q16 = reinterpret_cast<unsigned short *>(dispersion_q);
    const int k = s.count, k8 = (k + 7) & ~7;
    for (int i = tid; i < k8; i += kDispersionThreads) q16[i] = i < k ? (unsigned short)dispersion_position<kTable>(a, sig, s.begin + i) : (unsigned short)0;
    __syncthreads();
    double acc_sum = 0.0, acc_near = 0.0;
    for (int i = tid; i < k; i += kDispersionThreads) {
        const float *__restrict__ row = a.D + (size_t)q16[i] * (size_t)a.n_univ;
        double sum = 0.0;
        float m = __builtin_inff();
        for (int j0 = 0; j0 < k; j0 += 8) {
            const uint4 w = dispersion_q[j0 >> 3];      // (one address for the whole wave: a broadcast)
            const unsigned qq[4] = {w.x, w.y, w.z, w.w};
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[(qq[u >> 1] >> (16 * (u & 1))) & 0xFFFF];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int j = j0 + u;
                if (j < k && j != i) {
                    sum += (double)v[u];
                    m = v[u] < m ? v[u] : m;
                }
            }
        }
        acc_sum += sum;
        acc_near += (double)m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc_sum += __shfl_xor(acc_sum, o);
        acc_near += __shfl_xor(acc_near, o);
    }
    if (lane == 0) {
        wave_sum[tid >> 6] = acc_sum;
        wave_near[tid >> 6] = acc_near;
    }
    __syncthreads();
    if (tid == 0) {
        double t_sum = wave_sum[0], t_near = wave_near[0];
        for (int w = 1; w < kDispersionThreads / 64; w++) {
            t_sum += wave_sum[w];
            t_near += wave_near[w];
        }
        a.out[blockIdx.x] = st_dispersion_record{t_sum, t_near};
    }
}

// the sigma form (the taxa-labels null) and the table form (the swap null) of the three task kernels
__global__ __launch_bounds__(kDispersionThreads) void k_dispersion_tasks_packed(DispersionTaskArgs a) { dispersion_tasks_packed<false>(a); }
__global__ __launch_bounds__(kDispersionThreads) void k_dispersion_tasks_wave(DispersionTaskArgs a) { dispersion_tasks_wave<false>(a); }
__global__ __launch_bounds__(kDispersionThreads) void k_dispersion_tasks_group(DispersionTaskArgs a) { dispersion_tasks_group<false>(a); }
__global__ __launch_bounds__(kDispersionThreads) void k_swap_tasks_packed(DispersionTaskArgs a) { dispersion_tasks_packed<true>(a); }
__global__ __launch_bounds__(kDispersionThreads) void k_swap_tasks_wave(DispersionTaskArgs a) { dispersion_tasks_wave<true>(a); }
__global__ __launch_bounds__(kDispersionThreads) void k_swap_tasks_group(DispersionTaskArgs a) { dispersion_tasks_group<true>(a); }

}  // namespace st
