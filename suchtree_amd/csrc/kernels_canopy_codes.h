// kernels_canopy_codes.h -- k_canopy_ilp_codes: the predicated kernel on heap codes (tree_prep.h: prepare_heap_codes; perfect
// trees whose edge lengths are six-decimal numbers, the headline tree among them).  The kernel of kernels_canopy.h's
// heap_pairs with another table under it: the six lowest edges of a leaf's lineage come from ONE 128-byte line of 20-bit
// codes that serves 24 leaf slots -- 5.33 MiB for 2^20 leaves where the float lines take 8, so that three of four line
// lookups hit a 4 MiB L2 instead of two of four (scripts/l2_lru_model.py) --, the rest from the same heap image in LDS.
// Two loads per node as there (a 16-byte window and a 16-byte top, 4-byte aligned, neither leaves its line, shared between
// lanes l and l ^ 1 as there), every load and
// LDS read of a pair issued before anything uses one, k from sa ^ sb, sums from +0.0f, every add predicated with kChainPad,
// the reference's adds in the reference's order: the codes decode to the very floats the heap lines hold (the builder
// verified every edge), so the results are the same bits.  Instantiated in launch_canopy_codes.hip.
#pragma once
#include <type_traits>

#include "device_common.h"
#include "kernels_canopy.h"
#include "pair_math.h"
#include "tree_prep.h"

namespace st {

struct CodesParams {
    const uint32_t *codes;         // [ceil(2^(D-3) / 3) * 32] heap codes
    const float *dist;             // [heap_image_bytes(D) / 4] heap image, staged to LDS
    const Node8 *nodes;            // the walk family's tables (pairs with an internal node)
    const int32_t *depth;
    const Stride3 *stride;
    long long n_nodes;
    int32_t levels;                // D: edges between a leaf and the root
};

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
// heap_code_pair_word; HeapSide of kernels_canopy.h does the same on the float lines): either gather instruction reads the
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

// The kernel's loop over its pairs, NT: with the streaming hint on the pair load and the result stores (device_common.h), as
// in heap_pairs -- one of two copies of the loop, chosen once.
template <bool NT, typename Src>
__device__ __forceinline__ void codes_pairs(const CodesParams &P, const Src &src, long long n, const DistSink &out_d, const MrcaSink &out_m,
                                            Fault *fault, const float *H)
{
    const uint32_t first = 1u << (P.levels - kHeapLineEdges);      // heap index of slot block 0 at the lowest level of the image
    const float pad = __uint_as_float(kChainPad);
    const uint32_t odd = 0u - (threadIdx.x & 1u);      // the lane's parity as a mask (tree_prep.h: heap_pair_window_mask)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool live = i < n;
        long long ida, idb;
        src.template load_as<NT>(live ? i : n - 1, ida, idb);
        const bool valid = (unsigned long long)ida < (unsigned long long)P.n_nodes && (unsigned long long)idb < (unsigned long long)P.n_nodes;
        if (!valid && live) record_fault(fault, ida, idb, P.n_nodes);
        const bool leaves = valid && !((ida | idb) & 1);
        // (anything else reads slot 0 and is answered below: no address depends on an id that was not checked)
        const uint32_t sa = leaves ? (uint32_t)ida >> 1 : 0u, sb = leaves ? (uint32_t)idb >> 1 : 0u;
        // every load of both lines before anything uses them (converged: the lane pairs exchange slots here ...)
        CodeSide A, B;
        A.issue(P.codes, sa, odd);
        B.issue(P.codes, sb, odd);
        // ... and the heap entries of both lineages: index (first + (slot >> 6)) >> q for the q-th edge above the line (a
        // climb that is over, or a level the tree does not have, reads an entry that is never added: entry 1 at the least)
        const uint32_t ua = first + (sa >> kHeapLineEdges), ub = first + (sb >> kHeapLineEdges);
        float ha[kHeapClimbMax], hb[kHeapClimbMax];
#pragma unroll
        for (int q = 0; q < kHeapClimbMax; q++) {
            const uint32_t xa = ua >> q, xb = ub >> q;
            ha[q] = H[xa ? xa : 1u];
            hb[q] = H[xb ? xb : 1u];
        }
        const uint32_t x = sa ^ sb;
        const int k = x ? 32 - __clz((int)x) : 0;      // edges either side climbs
        A.settle(odd);                                 // (... and tops here: before the branch of the internal nodes)
        B.settle(odd);
        float s = A.add(0.0f, k);
#pragma unroll
        for (int q = 0; q < kHeapClimbMax; q++) s += kHeapLineEdges + q < k ? ha[q] : pad;
        s = B.add(s, k);
#pragma unroll
        for (int q = 0; q < kHeapClimbMax; q++) s += kHeapLineEdges + q < k ? hb[q] : pad;
        int m = k ? (int)((((((sa >> k) << 1) | 1u) << k)) - 1u) : (int)ida;
        if (valid && !leaves) {      // an internal node (rare)
            const PairResult r = pair_walk(P.nodes, P.depth, P.stride, (int32_t)ida, (int32_t)idb);
            s = r.dist;
            m = r.mrca;
        }
        // (converged: every lane of the workgroup is here, with consecutive pair numbers)
        store_result_wave_as<NT>(out_d, out_m, i, valid ? s : __builtin_nanf(""), valid ? m : -1, live);
    }
}

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
        if (src.nt) codes_pairs<true>(P, src, n, out_d, out_m, fault, H);
        else codes_pairs<false>(P, src, n, out_d, out_m, fault, H);
    } else {
        // the int32 source (the host path, never hinted by default) keeps the plain loop alone, as in k_canopy_ilp_heap
        codes_pairs<false>(P, src, n, out_d, out_m, fault, H);
    }
}

}  // namespace st
