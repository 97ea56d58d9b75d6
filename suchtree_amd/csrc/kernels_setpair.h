// kernels_setpair.h -- included by suchtree_hip.hip (after kernels_dispersion.h, whose sigma kernel and unroll it uses).
// The device side of st_beta_dispersion_host and st_beta_dispersion_matrix (layout: setpair_plan.h; the contract:
// include/suchtree_hip.h).  Task (r -> c, p) relabels both sets' positions through sigma_p and reduces the k_r x k_c
// sub-matrix D[q_a][q'_b] of the float32 matrix D: every row's sum and minimum over the included b, then both over a.
// The sigma rows are k_dispersion_sigma's, unchanged.
//
//   k_setpair_tasks_*   three forms, keyed on k_r; element a of a task is a lane's, the lane walks b:
//       packed     K' <= 32: 64 / K' tasks per wave.  The walked set is staged K' entries at a time, entry b0 + l in lane l
//                  of the task's group, and read from there as the dispersion kernel reads q_j; the wave walks to its
//                  longest k_c (the plan orders a class by k_c), the butterfly inside the group;
//       wave       33 <= k_r <= 64: one task per wave, 64 entries staged at a time, read at a wave-uniform b (a scalar);
//       workgroup  k_r > 64: 256 lanes, the whole walked set staged in LDS as uint16 (up to 32 KiB), eight q'_b per
//                  16-byte broadcast read; lane t takes the elements t, t + 256, ...
//     A staged entry is q'_b with the walked member's unpermuted position beside it (the high half of the lane's word;
//     a second uint16 array in LDS), compared with the lane's own position: exclude_shared leaves the equal one out.
//     Without exclude_shared the position is 0xFFFF, which no member has, and the workgroup form stages none.
//     A step issues kDispersionUnroll independent 4-byte gathers before the first add, then adds them in b order.
//
// Determinism: a row's sum runs over b ascending in one lane; the order over a is that of setpair_record
// (setpair_plan.cpp), operation for operation.  No float atomics.
#pragma once

#include "setpair_plan.h"

namespace st {

constexpr unsigned kSetpairNoPosition = 0xFFFFu;      // above every position of a universe of up to 2^14

struct SetpairTaskArgs {
    const float *D;
    const unsigned short *sigma;         // the block's rows
    const int *set_pos;
    const SetpairTaskDev *tasks;         // the live directions in plan order
    st_dispersion_record *out;           // this launch's records: entry `slot`
    long long task0, n;                  // this launch: n tasks (n < 2^31), the first one of direction task0 ...
    unsigned perm0, n_perms;             // ... under row perm0 of the block's n_perms: task slot is (task0, perm0) + slot, row-fastest
    int n_univ, lanes, exclude;          // packed form: K'
};

__device__ __forceinline__ void setpair_task(const SetpairTaskArgs &a, long long slot, SetpairTaskDev &t, const unsigned short *&sig)
{
    const unsigned u = a.perm0 + (unsigned)slot, c = u / a.n_perms;      // (32 bits: perm0 < n_perms < 2^25, slot < 2^31)
    t = a.tasks[a.task0 + c];
    sig = a.sigma + (size_t)(u - c * a.n_perms) * (size_t)a.n_univ;
}

// entry b of the walked set as a lane holds it: q'_b, the position beside it; past the set: row entry 0, no position
__device__ __forceinline__ unsigned setpair_entry(const SetpairTaskArgs &a, const SetpairTaskDev &t, const unsigned short *sig, int b)
{
    if (b >= t.c_count) return kSetpairNoPosition << 16;
    const int pc = a.set_pos[t.c_begin + b];
    return (unsigned)sig[pc] | ((a.exclude ? (unsigned)pc : kSetpairNoPosition) << 16);
}

// the lane has no included entry: decided by the sets
__device__ __forceinline__ bool setpair_none(const SetpairTaskArgs &a, const SetpairTaskDev &t, int own)
{
    return a.exclude && t.c_count == 1 && a.set_pos[t.c_begin] == own;
}

__global__ __launch_bounds__(kDispersionThreads) void k_setpair_tasks_packed(SetpairTaskArgs a)
{
    const int lane = threadIdx.x & 63, kp = a.lanes, li = lane & (kp - 1);
    const long long wave = (long long)blockIdx.x * (kDispersionThreads / 64) + (threadIdx.x >> 6);
    const long long slot = wave * (64 / kp) + lane / kp;      // (the lanes of a group agree)
    const bool task = slot < a.n;
    SetpairTaskDev t{0, 0, 0, 0};
    const unsigned short *sig = a.sigma;
    if (task) setpair_task(a, slot, t, sig);
    const bool live = task && li < t.r_count;
    const int own = live ? a.set_pos[t.r_begin + li] : 0;
    const int q = live ? (int)sig[own] : 0;      // (an absent lane reads row 0 and adds nothing)
    const bool none = live && setpair_none(a, t, own);
    const int group = lane - li, kc = t.c_count;
    int kmax = kc;      // every group walks the wave's longest set: the exchange needs all lanes of the wave
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o));
    double sum = 0.0;
    float m = __builtin_inff();
    const float *row = a.D + (size_t)q * (size_t)a.n_univ;
    for (int b0 = 0; b0 < kmax; b0 += kp) {
        const int pk = (int)setpair_entry(a, t, sig, b0 + li);
        for (int j0 = 0; j0 < kp; j0 += kDispersionUnroll) {
            unsigned w[kDispersionUnroll];
            float v[kDispersionUnroll];
#pragma unroll
            for (int u = 0; u < kDispersionUnroll; u++) {      // (K' is wave-uniform)
                w[u] = j0 + u < kp ? (unsigned)__shfl(pk, group + j0 + u) : kSetpairNoPosition << 16;
                v[u] = j0 + u < kp ? row[w[u] & 0xFFFF] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kDispersionUnroll; u++) {
                const int j = j0 + u;
                if (live && j < kp && b0 + j < kc && (w[u] >> 16) != (unsigned)own) {
                    sum += (double)v[u];
                    m = v[u] < m ? v[u] : m;
                }
            }
        }
    }
    double nearest = live && !none ? (double)m : 0.0;
    for (int o = kp >> 1; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        nearest += __shfl_xor(nearest, o);
    }
    if (task && li == 0) a.out[slot] = st_dispersion_record{sum, nearest};
}

__global__ __launch_bounds__(kDispersionThreads) void k_setpair_tasks_wave(SetpairTaskArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long slot = (long long)blockIdx.x * (kDispersionThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= a.n) return;      // (wave-uniform; no workgroup barrier below)
    SetpairTaskDev t;
    const unsigned short *sig;
    setpair_task(a, slot, t, sig);
    t = SetpairTaskDev{__builtin_amdgcn_readfirstlane(t.r_begin), __builtin_amdgcn_readfirstlane(t.r_count), __builtin_amdgcn_readfirstlane(t.c_begin),
                       __builtin_amdgcn_readfirstlane(t.c_count)};      // (scalars: the b loop is uniform)
    const bool live = lane < t.r_count;
    const int own = live ? a.set_pos[t.r_begin + lane] : 0;
    const int q = live ? (int)sig[own] : 0;
    const bool none = live && setpair_none(a, t, own);
    double sum = 0.0;
    float m = __builtin_inff();
    const float *__restrict__ row = a.D + (size_t)q * (size_t)a.n_univ;
    for (int b0 = 0; b0 < t.c_count; b0 += 64) {
        const int pk = (int)setpair_entry(a, t, sig, b0 + lane);
        const int kt = min(64, t.c_count - b0);
        for (int j0 = 0; j0 < kt; j0 += kDispersionUnroll) {
            unsigned w[kDispersionUnroll];
            float v[kDispersionUnroll];
#pragma unroll
            for (int u = 0; u < kDispersionUnroll; u++) {
                w[u] = (unsigned)__builtin_amdgcn_readlane(pk, min(j0 + u, kt - 1));
                v[u] = row[w[u] & 0xFFFF];
            }
#pragma unroll
            for (int u = 0; u < kDispersionUnroll; u++) {
                if (live && j0 + u < kt && (w[u] >> 16) != (unsigned)own) {
                    sum += (double)v[u];
                    m = v[u] < m ? v[u] : m;
                }
            }
        }
    }
    double nearest = live && !none ? (double)m : 0.0;
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        nearest += __shfl_xor(nearest, o);
    }
    if (lane == 0) a.out[slot] = st_dispersion_record{sum, nearest};
}

// the dynamic LDS of the workgroup form for a walked set of up to k positions: q' (and the positions) in whole 16-byte
// words, and room for the eight wave totals that reuse it
ST_QUARTET_HD size_t setpair_lds_bytes(int k, bool exclude)
{
    const size_t words = (((size_t)k + 7) & ~(size_t)7) * 2 * (exclude ? 2 : 1);
    return words < 64 ? 64 : words;
}

__global__ __launch_bounds__(kDispersionThreads) void k_setpair_tasks_group(SetpairTaskArgs a)
{
    extern __shared__ uint4 setpair_q[];      // q' as uint16, eight to a 16-byte read, padded with position 0; then the positions
    const int tid = threadIdx.x, lane = tid & 63;
    SetpairTaskDev t;
    const unsigned short *sig;
    setpair_task(a, blockIdx.x, t, sig);      // (workgroup-uniform)
    t = SetpairTaskDev{__builtin_amdgcn_readfirstlane(t.r_begin), __builtin_amdgcn_readfirstlane(t.r_count), __builtin_amdgcn_readfirstlane(t.c_begin),
                       __builtin_amdgcn_readfirstlane(t.c_count)};
    const int kr = t.r_count, kc = t.c_count, k8 = (kc + 7) & ~7;
    unsigned short *q16 = reinterpret_cast<unsigned short *>(setpair_q), *p16 = q16 + k8;
    for (int b = tid; b < k8; b += kDispersionThreads) {
        const int pc = b < kc ? a.set_pos[t.c_begin + b] : 0;
        q16[b] = b < kc ? sig[pc] : (unsigned short)0;
        if (a.exclude) p16[b] = b < kc ? (unsigned short)pc : (unsigned short)kSetpairNoPosition;
    }
    __syncthreads();
    const uint4 *positions = setpair_q + (k8 >> 3);
    double acc_sum = 0.0, acc_near = 0.0;
    for (int i = tid; i < kr; i += kDispersionThreads) {
        const int own = a.set_pos[t.r_begin + i];
        const float *__restrict__ row = a.D + (size_t)sig[own] * (size_t)a.n_univ;
        double sum = 0.0;
        float m = __builtin_inff();
        for (int j0 = 0; j0 < kc; j0 += 8) {
            const uint4 w = setpair_q[j0 >> 3];      // (one address for the whole wave: a broadcast)
            const uint4 s = a.exclude ? positions[j0 >> 3] : uint4{~0u, ~0u, ~0u, ~0u};
            const unsigned qq[4] = {w.x, w.y, w.z, w.w}, ss[4] = {s.x, s.y, s.z, s.w};
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = row[(qq[u >> 1] >> (16 * (u & 1))) & 0xFFFF];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (j0 + u < kc && ((ss[u >> 1] >> (16 * (u & 1))) & 0xFFFF) != (unsigned)own) {
                    sum += (double)v[u];
                    m = v[u] < m ? v[u] : m;
                }
            }
        }
        acc_sum += sum;
        acc_near += setpair_none(a, t, own) ? 0.0 : (double)m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc_sum += __shfl_xor(acc_sum, o);
        acc_near += __shfl_xor(acc_near, o);
    }
    __syncthreads();      // (every lane has read its last staged word: the wave totals take the place of the first ones)
    double *wave_sum = reinterpret_cast<double *>(setpair_q), *wave_near = wave_sum + kDispersionThreads / 64;
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

}  // namespace st
