// kernels_canopy_heap.h -- what the two heap-family kernels share: k_canopy_ilp_heap (kernels_canopy.h, on heap lines) and
// k_canopy_ilp_codes (kernels_canopy_codes.h, on heap codes) are ONE loop over the pairs, heap_pairs<NT, Side>, with two ways
// for a lane to get the six lowest edges of a leaf's lineage out of its 128-byte line (HeapSide below, CodeSide there).
//
// The predicated kernel on heap lines (tree_prep.h: prepare_heap_lines; perfect trees with in-order ids, the headline tree
// among them).  Ids are arithmetic there: leaf slots sa = a >> 1 and sb = b >> 1 part ways k = bit length of (sa ^ sb)
// edges below their MRCA, whose id is ((((sa >> k) << 1) | 1) << k) - 1; either side adds the six lowest edges of its
// lineage from ONE 128-byte line (the line of 16 leaf slots; of 24 where the line holds 20-bit codes) and the rest from
// the heap image in LDS, entry (2^(D-6) + (slot >> 6)) >> q for its q-th edge above the line.  No portal, no block table,
// no depth cut, no shared-portal case: one formula for every leaf pair, and a gather footprint of 8 MiB for 2^20 leaves
// (5.33 MiB of codes) where rec_a4 and the cherry records take 20.  None of the addresses depends on a load but the
// pair's own, so a lane issues its four line loads (two 16-byte loads per node: Side::issue) and all its LDS reads at
// once.  Four, because with eight narrower loads on a line per 16 leaves in level order the kernel ran at the old 2.80 ms
// per 1e8 pairs: L1-miss latency per pair fell by 19 % but the vector-memory address pipeline stayed busy 93 % of the
// launch (LAB_NOTES.md 9).  Sums start at +0.0f and every add is predicated with -0.0f (kChainPad) as in k_canopy_ilp: the
// reference's adds in the reference's order, the same bits.  A pair with an internal node (odd id) is walked on the tree
// itself (rare: a wave-level branch).
//
// A Side is the line part of one leaf slot's lineage: issue(table, slot, odd) starts its two loads, settle(odd) sorts out
// what the lane pair l, l ^ 1 loaded for each other (every lane of the wave must be active in both), add(s, k) adds the
// first min(k, 6) edges to s in order.
#pragma once
#include "device_common.h"
#include "launch_geometry.h"
#include "pair_math.h"
#include "tree_prep.h"

namespace st {

template <typename Word>
struct HeapParamsT {
    const Word *lines;             // float: [2^(D-4) * 32] heap lines; uint32_t: [ceil(2^(D-3) / 3) * 32] heap codes
    const float *dist;             // [heap_image_bytes(D) / 4] heap image, staged to LDS
    const Node8 *nodes;            // the walk family's tables (pairs with an internal node)
    const int32_t *depth;
    const Stride3 *stride;
    long long n_nodes;
    int32_t levels;                // D: edges between a leaf and the root
};
using HeapParams = HeapParamsT<float>;
using CodesParams = HeapParamsT<uint32_t>;
constexpr int kHeapLineEdges = 6;                                   // edges of a lineage that its line holds
constexpr int kHeapClimbMax = kHeapMaxLevels - kHeapLineEdges;      // ... and the most that are left for the heap image

typedef float __attribute__((ext_vector_type(4), aligned(4))) float4_align4;      // a 16-byte load at any dword

// The six line values of one leaf slot (tree_prep.h: the layout of a heap line) out of two 16-byte loads, the window of the
// slot's group of four leaves and the line's last four floats -- shared between lanes l and l ^ 1 (tree_prep.h:
// heap_pair_offset): either gather instruction reads the window of one of the two slots on its own lane and the top of the same
// slot on the lane beside it, so the L1 looks every line up once (a lane that read both had its second lookup behind those of
// the 63 other lanes, and 0.18 requests per pair went out again for a tag replaced in between).  The loading lane picks the
// neighbour's e3 and hands the three top values over by quad permutes: no LDS, and every lane of the wave must be active.
__device__ __forceinline__ uint32_t heap_lane_swap(uint32_t v)      // lane l reads lane l ^ 1 (quad_perm:[1,0,3,2])
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}
struct HeapSide {
    float4_align4 w;       // issue(): the loads of step 0 and 1; settle(): the slot's own window
    float4_align4 top;     // issue(): ...; settle(): x, y, z = the slot's e3, e4, e5
    uint32_t t, nb;
    // odd: all ones on an odd lane, 0 on an even one
    __device__ __forceinline__ void issue(const float *lines, uint32_t sl, uint32_t odd)
    {
        t = sl & 15u;
        nb = heap_lane_swap(sl);
        w = *reinterpret_cast<const float4_align4 *>(lines + heap_pair_offset(0, odd, sl, nb));
        top = *reinterpret_cast<const float4_align4 *>(lines + heap_pair_offset(1, odd, sl, nb));
    }
    __device__ __forceinline__ void settle(uint32_t odd)
    {
        const uint32_t m = heap_pair_window_mask(1, odd);      // set: step 1 read the own window and step 0 the neighbour's top
        const uint32_t a0 = __float_as_uint(w.x), a1 = __float_as_uint(w.y), a2 = __float_as_uint(w.z), a3 = __float_as_uint(w.w);
        const uint32_t b0 = __float_as_uint(top.x), b1 = __float_as_uint(top.y), b2 = __float_as_uint(top.z), b3 = __float_as_uint(top.w);
        w.x = __uint_as_float(heap_pair_select(m, b0, a0));
        w.y = __uint_as_float(heap_pair_select(m, b1, a1));
        w.z = __uint_as_float(heap_pair_select(m, b2, a2));
        w.w = __uint_as_float(heap_pair_select(m, b3, a3));
        const uint32_t n0 = heap_pair_select(m, a0, b0), n3 = heap_pair_select(m, a3, b3);      // the neighbour's top
        top.x = __uint_as_float(heap_lane_swap((nb & 8u) ? n3 : n0));
        top.y = __uint_as_float(heap_lane_swap(heap_pair_select(m, a1, b1)));
        top.z = __uint_as_float(heap_lane_swap(heap_pair_select(m, a2, b2)));
    }
    // s += the first k (at most six) of the leaf's edges, in order; every add predicated (kChainPad)
    __device__ __forceinline__ float add(float s, int k) const
    {
        const float pad = __uint_as_float(kChainPad);
        // (selects between pairs of components only: a select chain over all four components of one vector can become an
        // extract at a variable index, which the compiler keeps in scratch memory -- tests/test_heap_kernel_resources.py)
        const float w0 = w.x, w1 = w.y, w2 = w.z, w3 = w.w;
        const bool hi = (t & 2u) != 0, odd = (t & 1u) != 0;
        const float own_lo = odd ? w1 : w0, own_hi = odd ? w3 : w2;
        s += 0 < k ? (hi ? own_hi : own_lo) : pad;
        s += 1 < k ? (hi ? w1 : w2) : pad;
        s += 2 < k ? (hi ? w0 : w3) : pad;
        s += 3 < k ? top.x : pad;
        s += 4 < k ? top.y : pad;
        s += 5 < k ? top.z : pad;
        return s;
    }
};

// The kernels' loop over their pairs, NT: with the streaming hint on the pair load and the result stores (device_common.h).  The hint
// is a run-time field, but this loop has no scalar register to spare for one more loop-invariant condition (the plain form sits at
// the limit; tests/test_heap_kernel_resources.py), so a kernel tests it once and runs one of two copies of the loop.
template <bool NT, typename Side, typename Word, typename Src>
__device__ __forceinline__ void heap_pairs(const HeapParamsT<Word> &P, const Src &src, long long n, const DistSink &out_d,
                                           const MrcaSink &out_m, Fault *fault, const float *H)
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
        Side A, B;
        A.issue(P.lines, sa, odd);
        B.issue(P.lines, sb, odd);
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
        A.settle(odd);                                 // (... and top values here: before the branch of the internal nodes)
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

}  // namespace st
