// device_common.h -- included first by every translation unit of libsuchtree_hip.so.
// Fault word, pair sources (where pair i of a launch comes from), result sinks.
#pragma once
#include "compare_plan.h"

namespace st {

// --------------------------------------------------------------------------
// device-side helpers
// --------------------------------------------------------------------------
struct Fault {
    long long max_bad;   // largest offending id seen  (init INT64_MIN)
    long long min_bad;   // smallest offending id seen (init INT64_MAX)
};

__device__ __forceinline__ void record_fault(Fault *f, long long a, long long b, long long n_nodes)
{
    if (a < 0 || a >= n_nodes) { atomicMax(&f->max_bad, a); atomicMin(&f->min_bad, a); }
    if (b < 0 || b >= n_nodes) { atomicMax(&f->max_bad, b); atomicMin(&f->min_bad, b); }
}

// ---- the streaming hint ----------------------------------------------------
// A pair array is read once and a result array written once, yet their lines allocate in L2 and push out the table lines
// a kernel gathers from: on the 8 MiB of heap lines behind a 4 MiB L2 the 28 bytes per pair of the headline launch cost
// one fabric read in ten (scripts/l2_lru_model.py; LAB_NOTES.md 9).  `nt` of an explicit pair source marks the launch's
// pair array and result arrays as such streams: the loads of the pairs then carry the non-temporal modifier
// (global_load_dwordx4 ... nt) and, in k_canopy_ilp_heap, so do the stores of the results (global_store_dword ... nt).
// A run-time, wave-uniform field like SrcContig32::packed48, so that no kernel is compiled twice; the host sets it
// (launch_policy.h: stream_hint_applies) and aggregate initialisation without it leaves it 0.  The same bytes at the
// same addresses either way.  The sinks carry no field of their own: k_canopy_ilp_heap sits at its limit of scalar
// registers (tests/test_heap_kernel_resources.py allows no spill), and one more word among its arguments, or one more
// loop-invariant condition in its loop, makes it spill -- so that kernel tests the source's field once and runs one of two
// copies of its loop (kernels_canopy_heap.h: heap_pairs), and the other kernels' stores stay plain.  load() stays the plain load:
// only k_canopy_ilp, measured with it, asks for load_stream(); every other kernel compiles to what it was.
// A hinted access and its plain twin sit in the two arms of a branch, same address, same value: the optimiser hoists or sinks them
// into ONE access and, the hint being advice, drops it on the way (seen on the pair load and on both id stores of
// k_canopy_ilp_heap; a compiler fence between them does not stop it).  It merges only accesses that are the same operation, and
// the declared alignment is part of that: the hinted ones go through types that claim HALF their natural alignment (claiming
// less than holds is always allowed, and global memory takes a dword or a 16-byte access at any such address in one instruction:
// HeapSide's float4_align4).  tests/test_stream_hint_codegen.py notices if the hint gets lost again.
typedef long long __attribute__((ext_vector_type(2), aligned(8))) StreamI64x2;
typedef int __attribute__((ext_vector_type(2), aligned(4))) StreamI32x2;
typedef int __attribute__((aligned(2))) StreamI32;
typedef unsigned __attribute__((aligned(2))) StreamU32;
typedef float __attribute__((aligned(2))) StreamF32;
typedef double __attribute__((aligned(4))) StreamF64;

// ---- pair sources: where pair number i of a launch comes from ----------------
// C-order int64 (n,2): one 16-byte load per lane, fully coalesced.
struct SrcContig {
    const long long *pairs;
    int nt;      // the streaming hint (above)
    template <bool NT> __device__ __forceinline__ void load_as(long long i, long long &a, long long &b) const
    {
        if constexpr (NT) {
            const StreamI64x2 v = __builtin_nontemporal_load(reinterpret_cast<const StreamI64x2 *>(pairs) + i);
            a = v.x;
            b = v.y;
        } else {
            const longlong2 v = reinterpret_cast<const longlong2 *>(pairs)[i];
            a = v.x;
            b = v.y;
        }
    }
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const { load_as<false>(i, a, b); }
    // with the hint where the field says so: the kernels that were measured with it (k_canopy_ilp; kernels_canopy.h: load_pair)
    __device__ __forceinline__ void load_stream(long long i, long long &a, long long &b) const
    {
        if (nt) load_as<true>(i, a, b);
        else load_as<false>(i, a, b);
    }
};

// C-order int32 (n,2): what the host path ships over PCIe (node ids always fit in 31 bits;
// the packing step clamps anything wider so that it still fails the range check).
// packed48: the narrower wire format of trees with fewer than 2^24 nodes -- 24 bits per id, 6 bytes per pair, three
// 2-byte loads per lane (consecutive lanes read consecutive bytes; 0xFFFFFF stands for an id out of range, which the
// host has already judged: host_copy.h::pack_pairs48).  One type for both formats (a wave-uniform branch), so that
// no kernel is compiled twice for it.  (nt: the 8-byte form only; the packed form keeps its plain 2-byte loads.)
struct SrcContig32 {
    const int *pairs;
    int packed48;
    int nt;      // the streaming hint (above); sits in what was padding
    // NT: the hinted load of the 8-byte form (the caller has checked that the source is not packed)
    template <bool NT> __device__ __forceinline__ void load_as(long long i, long long &a, long long &b) const
    {
        if constexpr (NT) {
            const StreamI32x2 v = __builtin_nontemporal_load(reinterpret_cast<const StreamI32x2 *>(pairs) + i);
            a = v.x;
            b = v.y;
        } else if (packed48) {
            const unsigned short *q = reinterpret_cast<const unsigned short *>(pairs) + 3 * i;
            const unsigned w0 = q[0], w1 = q[1], w2 = q[2];
            a = (long long)(w0 | ((w1 & 0xFFu) << 16));
            b = (long long)((w1 >> 8) | (w2 << 8));
        } else {
            const int2 v = reinterpret_cast<const int2 *>(pairs)[i];
            a = v.x;
            b = v.y;
        }
    }
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const { load_as<false>(i, a, b); }
    __device__ __forceinline__ void load_stream(long long i, long long &a, long long &b) const      // (see SrcContig)
    {
        if (nt && !packed48) load_as<true>(i, a, b);
        else load_as<false>(i, a, b);
    }
};

// Any other (n,2) view: element strides s0 (rows) and s1 (columns).
struct SrcStrided {
    const long long *pairs;
    long long s0, s1;
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        a = pairs[i * s0];
        b = pairs[i * s0 + s1];
    }
};

// All-pairs generator: pair k = (ids[j], ids[i]) with k = i(i-1)/2 + j, 0 <= j < i,
// the enumeration of SuchLinkedTrees.linked_distances (MuchTree.pyx:2918-2925) and, up to
// order, of pairwise_distances (:1111-1114).  Nothing is read but the id list: within a
// wave b = ids[i] is (nearly) uniform and a = ids[j] walks the list, so the record reads
// of consecutive lanes fall on consecutive sectors.
struct SrcTriangle {
    const long long *ids;
    long long stride;   // element stride of ids
    long long k0;       // first pair index of this launch
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        const long long k = k0 + i;
        long long row = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
        if (row * (row - 1) / 2 > k) row--;
        if ((row + 1) * row / 2 <= k) row++;
        const long long col = k - row * (row - 1) / 2;
        a = ids[col * stride];
        b = ids[row * stride];
    }
};

// Clade segments (st_compare_clades_host): pair k lies in one segment of a clade plan -- a rectangle (rows x cols of
// link positions) or a triangle (all pairs within rows) -- and is evaluated as (lower rank, higher rank).  `ids` is this
// tree's node id per link position (links permuted so that every clade is one range), `rank` each position's rank.
// The segment of k is found by a binary search over the segments that meet k's tile of 2^kCladeTileShift pairs only
// (tile[t].seg = the segment of pair t * 2^kCladeTileShift): one or two steps inside a large segment, at most
// kCladeTileShift + 1 among tiny ones -- never one over all segments.  seg[] ends with a sentinel whose first = the
// pair count.  Within a segment consecutive lanes share a row and walk the columns, as in the triangle.  (CladeSeg,
// CladeTile and kCladeTileShift: compare_plan.h, where the host fills them.)
struct SrcSegments {
    const int *ids;
    const int *rank;
    const CladeSeg *seg;
    const CladeTile *tile;
    long long k0;          // first pair index of this launch
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        const long long k = k0 + i;
        const long long t = k >> kCladeTileShift;
        int lo = tile[t].seg, hi = tile[t + 1].seg;      // largest s in [lo, hi] with seg[s].first <= k
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg[mid].first <= k) lo = mid;
            else hi = mid - 1;
        }
        const CladeSeg g = seg[lo];
        const long long l = k - g.first;
        int p, q;
        if (g.c0 >= 0) {
            const long long nc = g.c1 - g.c0;
            long long r = (long long)((double)l / (double)nc);
            if (r * nc > l) r--;
            else if ((r + 1) * nc <= l) r++;
            p = g.r0 + (int)r;
            q = g.c0 + (int)(l - r * nc);
        } else {      // (the enumeration of SrcTriangle)
            long long row = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)l)) * 0.5);
            if (row * (row - 1) / 2 > l) row--;
            if ((row + 1) * row / 2 <= l) row++;
            p = g.r0 + (int)(l - row * (row - 1) / 2);
            q = g.r0 + (int)row;
        }
        if (rank[p] > rank[q]) { const int s = p; p = q; q = s; }
        a = ids[p];
        b = ids[q];
    }
};

// Rows of id lists (st_compare_rows_host): row r's pairs are the triangle over its m ids, P = m(m-1)/2 of them, pair k of
// row r at global index r * S + k (S = P, or P rounded up to a multiple of 2^kCladeTileShift; pairs [P, S) are padding
// and evaluate the row's first pair).  `ids` holds the rows uploaded for this chunk, from row r_base on.  r = g / S by a
// double reciprocal and a +-1 correction (global indices stay below 2^50), never a 64-bit divide per pair.
struct SrcRows {
    const int *ids;
    long long m, P, S;
    double inv_s;          // 1.0 / S
    long long k0;          // first global pair index of this launch
    long long r_base;      // the row at ids[0]
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        const long long g = k0 + i;
        long long r = (long long)((double)g * inv_s);
        if (r * S > g) r--;
        else if ((r + 1) * S <= g) r++;
        long long k = g - r * S;
        if (k >= P) k = 0;
        long long row = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);      // (the enumeration of SrcTriangle)
        if (row * (row - 1) / 2 > k) row--;
        if ((row + 1) * row / 2 <= k) row++;
        const int *v = ids + (r - r_base) * m;
        a = v[k - row * (row - 1) / 2];
        b = v[row];
    }
};

// Grid generator: element e = e0 + i of an n_rows x n_cols grid (C order) is the pair
// (rows[r], cols[c]), r = e / n_cols, c = e % n_cols.  `symmetric` (rows and cols are the same
// id list): below the diagonal the pair is taken in the order of its mirror image above it,
// (ids[c], ids[r]) for c < r, so the square is exactly the mirrored upper triangle that
// pairwise_distances builds (MuchTree.pyx:1106-1124: d(ids[i], ids[j]) for i < j, stored at
// [i,j] and [j,i]); the diagonal comes out as d(x,x) = 0.  Consecutive lanes share one endpoint
// and walk the id list with the other, so record reads coalesce as in the triangle.
struct SrcGrid {
    const long long *rows, *cols;
    long long n_cols, e0;
    int symmetric;
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        const long long e = e0 + i;
        const long long r = e / n_cols, c = e - r * n_cols;
        a = rows[r];
        b = cols[c];
        if (symmetric && c < r) { const long long t = a; a = b; b = t; }
    }
};

// Where distances go.  The C ABI's contract is float64 (what the reference returns); the
// values are float32 sums, so the host path ships them over PCIe as float32 and widens them
// on the host (half the D2H bytes, bit-identical result).
struct DistSink {
    double *d64;
    float *f32;
    __host__ __device__ bool any() const { return d64 != nullptr || f32 != nullptr; }
};

// The six pairs of a quartet (a,b,c,d), in the reference's order ab ac ad bc bd cd
// (MuchTree.pyx:1353-1358): pair i is combination i % 6 of quartet i / 6.  Lets the canopy
// kernels produce the six MRCA ids of every quartet without a pair array.
struct SrcQuartet {
    const long long *q;   // C-order int64 (n,4)
    __device__ __forceinline__ void load(long long i, long long &a, long long &b) const
    {
        const long long quartet = i / 6;
        const int combo = (int)(i - quartet * 6);
        const int ia = (0x940 >> (2 * combo)) & 3;    // 0 0 0 1 1 2
        const int ib = (0xFB9 >> (2 * combo)) & 3;    // 1 2 3 2 3 3
        a = q[quartet * 4 + ia];
        b = q[quartet * 4 + ib];
    }
};

// Where MRCA ids go: int32 per pair, or -- the host path's way back on trees of fewer than 2^24 nodes -- 24 bits
// per pair: pair i at bytes [3 i, 3 i + 3), little endian, -1 (an id out of range) as 0xFFFFFF; the buffer is padded
// to a multiple of four bytes.  7 instead of 8 bytes per pair then cross the link with the float32 distance
// (scripts/micro/link_pack_bench.hip: +13 % on the link side; host_copy.h::unpack_ids24 widens them again).
struct MrcaSink {
    int *m32;
    unsigned char *m24;
    __host__ __device__ bool any() const { return m32 != nullptr || m24 != nullptr; }
};

// Plain (NT = false) or hinted stores of one value (the under-aligned types: see the streaming hint above)
template <bool NT> __device__ __forceinline__ void stream_store(int *p, int v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<StreamI32 *>(p));
    else *p = v;
}
template <bool NT> __device__ __forceinline__ void stream_store(unsigned *p, unsigned v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<StreamU32 *>(p));
    else *p = v;
}
template <bool NT> __device__ __forceinline__ void stream_store(float *p, float v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<StreamF32 *>(p));
    else *p = v;
}
template <bool NT> __device__ __forceinline__ void stream_store(double *p, double v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<StreamF64 *>(p));
    else *p = v;
}

// One id, from any lane in any control flow (scattered form): three byte stores in the packed format.
template <bool NT> __device__ __forceinline__ void store_mrca_as(const MrcaSink &out, long long i, int m)
{
    if (out.m32) {
        stream_store<NT>(out.m32 + i, m);
    } else if (out.m24) {
        unsigned char *p = out.m24 + 3 * i;
        p[0] = (unsigned char)m;
        p[1] = (unsigned char)(m >> 8);
        p[2] = (unsigned char)(m >> 16);
    }
}
__device__ __forceinline__ void store_mrca(const MrcaSink &out, long long i, int m)
{
    store_mrca_as<false>(out, i, m);
}

// The ids of 64 consecutive pairs, one per lane: EVERY lane of the wave calls this in converged control flow with
// i = (a multiple of 4) + lane; lanes without a pair pass live = false.  Packed format: the four ids of a quad are
// twelve bytes = three dwords, assembled with one quad permute (lane p takes the id of lane p + 1) and stored by the
// quad's first three lanes -- a wave writes 192 consecutive bytes in aligned dwords, no byte stores (byte-masked
// partial writes are what a link to host memory handles worst).  A dword's upper bytes belong to the next pair: if
// that one is not live (the tail of a batch) or its id is not known yet (it follows by store_mrca) they are zero.
template <bool NT> __device__ __forceinline__ void store_mrca_wave_as(const MrcaSink &out, long long i, int m, bool live)
{
    if (out.m32) {
        if (live) stream_store<NT>(out.m32 + i, m);
    } else if (out.m24) {
        const unsigned v = live ? ((unsigned)m & 0xFFFFFFu) : 0u;
        const unsigned next = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9 /* quad_perm:[1,2,3,3] */, 0xF, 0xF, true);
        const unsigned p = (unsigned)i & 3u;
        if (live && p != 3u) {
            const unsigned w = (v >> (8u * p)) | (next << (24u - 8u * p));
            stream_store<NT>(reinterpret_cast<unsigned *>(out.m24) + (i >> 2) * 3 + p, w);
        }
    }
}
__device__ __forceinline__ void store_mrca_wave(const MrcaSink &out, long long i, int m, bool live)
{
    store_mrca_wave_as<false>(out, i, m, live);
}

template <bool NT> __device__ __forceinline__ void store_dist_as(const DistSink &out_d, long long i, float d)
{
    if (out_d.d64) stream_store<NT>(out_d.d64 + i, (double)d);
    else if (out_d.f32) stream_store<NT>(out_d.f32 + i, d);
}
__device__ __forceinline__ void store_dist(const DistSink &out_d, long long i, float d)
{
    store_dist_as<false>(out_d, i, d);
}

// scattered form (any lane, any control flow)
__device__ __forceinline__ void store_result(const DistSink &out_d, const MrcaSink &out_m, long long i, float d, int m)
{
    store_dist(out_d, i, d);
    store_mrca(out_m, i, m);
}

// converged form (see store_mrca_wave); NT: with the streaming hint (k_canopy_ilp_heap)
template <bool NT>
__device__ __forceinline__ void store_result_wave_as(const DistSink &out_d, const MrcaSink &out_m, long long i, float d, int m, bool live)
{
    if (live) store_dist_as<NT>(out_d, i, d);
    store_mrca_wave_as<NT>(out_m, i, m, live);
}
__device__ __forceinline__ void store_result_wave(const DistSink &out_d, const MrcaSink &out_m, long long i, float d, int m, bool live)
{
    store_result_wave_as<false>(out_d, out_m, i, d, m, live);
}

}  // namespace st
