// kernels_canopy_codes.h -- k_canopy_ilp_codes: the predicated kernel on heap codes (tree_prep.h: prepare_heap_codes; perfect
// trees whose edge lengths are six-decimal numbers, the headline tree among them).  heap_pairs of kernels_canopy_heap.h
// with another table under it (CodeSide): the six lowest edges of a leaf's lineage come from ONE 128-byte line of 20-bit
// codes that serves 24 leaf slots -- 5.33 MiB for 2^20 leaves where the float lines take 8, so that three of four line
// lookups hit a 4 MiB L2 instead of two of four (scripts/l2_lru_model.py) --, the rest from the same heap image in LDS.
// Two loads per node as there (a 16-byte window and a 16-byte top, 4-byte aligned, neither leaves its line, shared between
// lanes l and l ^ 1 as there), every load and
// LDS read of a pair issued before anything uses one, k from sa ^ sb, sums from +0.0f, every add predicated with kChainPad,
// the reference's adds in the reference's order: the codes decode to the very floats the heap lines hold (the builder
// verified every edge), so the results are the same bits.  Instantiated in launch_canopy_codes.hip.
#pragma once
#include <type_traits>

#include "kernels_canopy_heap.h"

namespace st {

typedef uint32_t __attribute__((ext_vector_type(4), aligned(4))) uint4_align4;      // a 16-byte load at any dword
typedef float __attribute__((ext_vector_type(2))) float2_v;

// heap_code_decode_f32 (tree_prep.h) of two codes at once: the same four float32 operations per code, two lanes of the packed
// instructions (v_pk_mul_f32, v_pk_fma_f32); explicit fused operations, as there
__device__ __forceinline__ float2_v heap_code_decode2(uint32_t c0, uint32_t c1)
{
    const float2_v f = {(float)c0, (float)c1};
    const float2_v q = f * (float2_v)(1e-6f);
    const float2_v r = __builtin_elementwise_fma(-q, (float2_v)(1e6f), f);
    return __builtin_elementwise_fma(r, (float2_v)(1e-6f), q);
}

// The six line values of one leaf slot out of two 16-byte loads shared between lanes l and l ^ 1 (tree_prep.h:
// heap_code_pair_word; HeapSide of kernels_canopy_heap.h does the same on the float lines): either gather instruction reads the
// window of one of the two slots on its own lane and the top of the same slot on the lane beside it, so the L1 looks every
// line up once (with every lane loading the window and the top of its own slot 0.45 of 2.58 L1-miss requests per pair were
// second lookups of a line).  The loading lane shifts the neighbour's top down to its 60 bits and hands two dwords over by
// quad permutes: no LDS, and every lane of the wave must be active in issue() and settle().  The codes are cut out by funnel
// shifts on fixed register pairs and selects between two candidates (tree_prep.h), never a dword at a variable position.
struct CodeSide {
    uint4_align4 a, b;      // issue(): the loads of step 0 and 1; settle(): a = the slot's own window, b.x, b.y = the 60 bits of its top
    uint32_t sl, pw, pt;    // the slot, the phase of its window and the phase of the NEIGHBOUR's top
    // odd: all ones on an odd lane, 0 on an even one
    __device__ __forceinline__ void issue(const uint32_t *codes, uint32_t slot, uint32_t odd)
    {
        sl = slot;
        const uint32_t nb = heap_lane_swap(slot);
        pw = heap_code_window_place(slot).phase;
        pt = heap_code_top_place(nb).phase;
        a = *reinterpret_cast<const uint4_align4 *>(codes + heap_code_pair_word(0, odd, slot, nb));
        b = *reinterpret_cast<const uint4_align4 *>(codes + heap_code_pair_word(1, odd, slot, nb));
    }
    __device__ __forceinline__ void settle(uint32_t odd)
    {
        const uint32_t m = heap_pair_window_mask(1, odd);      // set: step 1 read the own window and step 0 the neighbour's top
        const uint32_t t0 = heap_pair_select(m, a.x, b.x), t1 = heap_pair_select(m, a.y, b.y), t2 = heap_pair_select(m, a.z, b.z),
                       t3 = heap_pair_select(m, a.w, b.w);
        a.x = heap_pair_select(m, b.x, a.x);
        a.y = heap_pair_select(m, b.y, a.y);
        a.z = heap_pair_select(m, b.z, a.z);
        a.w = heap_pair_select(m, b.w, a.w);
        const HeapCodeTopBits n = heap_code_top_bits(t0, t1, t2, t3, pt);
        b.x = heap_lane_swap(n.n0);
        b.y = heap_lane_swap(n.n1);
    }
    // s += the first k (at most six) of the leaf's edges, in order; every add predicated (kChainPad)
    __device__ __forceinline__ float add(float s, int k) const
    {
        const float pad = __uint_as_float(kChainPad);
        const HeapCodeTriple lo = heap_code_window_fields(a.x, a.y, a.z, a.w, pw, sl);
        const HeapCodeTriple hi = heap_code_top_fields(b.x, b.y);
        const float2_v e01 = heap_code_decode2(lo.c0, lo.c1), e23 = heap_code_decode2(lo.c2, hi.c0), e45 = heap_code_decode2(hi.c1, hi.c2);
        s += 0 < k ? e01.x : pad;
        s += 1 < k ? e01.y : pad;
        s += 2 < k ? e23.x : pad;
        s += 3 < k ? e23.y : pad;
        s += 4 < k ? e45.x : pad;
        s += 5 < k ? e45.y : pad;
        return s;
    }
};

template <typename Src>
__global__ __launch_bounds__(kCanopyBlock, 4) void k_canopy_ilp_codes(CodesParams P, Src src, long long n, DistSink out_d,
                                                                      MrcaSink out_m, Fault *fault)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const float *H = reinterpret_cast<const float *>(lds_raw);
    {      // stage the heap image: 16 bytes per lane per step, coalesced
        const int n16 = (int)(heap_image_bytes(P.levels) / 16);
        const uint4 *src16 = reinterpret_cast<const uint4 *>(P.dist);
        uint4 *dst16 = reinterpret_cast<uint4 *>(lds_raw);
        for (int k = threadIdx.x; k < n16; k += blockDim.x) dst16[k] = src16[k];
        __syncthreads();
    }
    if constexpr (std::is_same<Src, SrcContig>::value) {
        if ((long long)blockIdx.x * blockDim.x >= n) return;
        if (src.nt) heap_pairs<true, CodeSide>(P, src, n, out_d, out_m, fault, H);
        else heap_pairs<false, CodeSide>(P, src, n, out_d, out_m, fault, H);
    } else {
        // the int32 source (the host path, never hinted by default) keeps the plain loop alone, as in k_canopy_ilp_heap
        heap_pairs<false, CodeSide>(P, src, n, out_d, out_m, fault, H);
    }
}

}  // namespace st
