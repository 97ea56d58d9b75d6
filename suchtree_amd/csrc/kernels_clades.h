// kernels_clades.h -- included by suchtree_hip.hip (after device_common.h and kernels_compare.h).
// The reduction of st_compare_clades_host: pair k has a float32 distance x[k] in tree X and y[k] in tree Y, written by
// the unchanged distance kernels over SrcSegments into compare_run's two scratch chunks.  The pair range is cut into
// tiles of 2^kCladeTileShift pairs aligned to global k (chunks are whole tiles); a piece is one segment's part of one
// tile.  This kernel writes the shifted float64 sums and the min / max of every piece (CladePiece, compare_plan.h); the
// host merges pieces into segments and segments into clades (compare_plan.cpp: clade_fold).
//
// Determinism: a piece is summed about its own first pair (cx, cy) = (x, y) of that pair, so it needs nothing from
// another tile or chunk, and in one order that depends on its length alone -- up to kCladeLanePiece pairs by one lane
// in index order, longer ones by one wave (lane l takes pairs l, l + 64, ... in order, then an xor butterfly, lane 0's
// result).  No float atomics; neither the grid nor the chunk size changes a piece, so neither changes a result.
#pragma once

namespace st {

constexpr int kCladeThreads = 256;        // four waves per workgroup, one tile per wave
constexpr int kCladeLanePiece = 64;       // pieces of at most this many pairs are summed by a single lane

struct CladeAcc {
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    float min_x = __builtin_huge_valf(), max_x = -__builtin_huge_valf();
    float min_y = __builtin_huge_valf(), max_y = -__builtin_huge_valf();

    __device__ __forceinline__ void add(float xf, float yf, double cx, double cy)
    {
        const double dx = (double)xf - cx, dy = (double)yf - cy;
        sx += dx;
        sy += dy;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
        min_x = fminf(min_x, xf);
        max_x = fmaxf(max_x, xf);
        min_y = fminf(min_y, yf);
        max_y = fmaxf(max_y, yf);
    }
};

__device__ __forceinline__ float clade_shift(float v) { return isfinite(v) ? v : 0.0f; }

__device__ __forceinline__ void clade_store(CladePiece *out, const CladeAcc &a, float cx, float cy)
{
    *out = CladePiece{a.sx, a.sy, a.sxx, a.syy, a.sxy, cx, cy, a.min_x, a.max_x, a.min_y, a.max_y};
}

// The wave's part of the order rule: lane l's sums combined by an xor butterfly over the 64 lanes (every lane ends with
// the same result; lane 0's is stored).  Shared by k_clade_pieces and k_row_blocks (kernels_rows.h).
__device__ __forceinline__ void clade_wave_reduce(CladeAcc &a)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.sx += __shfl_xor(a.sx, o);
        a.sy += __shfl_xor(a.sy, o);
        a.sxx += __shfl_xor(a.sxx, o);
        a.syy += __shfl_xor(a.syy, o);
        a.sxy += __shfl_xor(a.sxy, o);
        a.min_x = fminf(a.min_x, __shfl_xor(a.min_x, o));
        a.max_x = fmaxf(a.max_x, __shfl_xor(a.max_x, o));
        a.min_y = fminf(a.min_y, __shfl_xor(a.min_y, o));
        a.max_y = fmaxf(a.max_y, __shfl_xor(a.max_y, o));
    }
}

// One chunk: pairs [off, off + c) at x[0..c), y[0..c); off is a multiple of the tile.  Wave w of workgroup b takes tile
// (off >> kCladeTileShift) + 4 b + w; its pieces are segments tile[t].seg, tile[t].seg + 1, ... (every segment holds
// at least one pair), written to out[tile[t].piece + j].  Rounds of 64 pieces: lane j sums piece j if it is short, then
// the wave sums the long ones of the round together, in piece order.
__global__ __launch_bounds__(kCladeThreads) void k_clade_pieces(const float *__restrict__ x, const float *__restrict__ y, long long off,
                                                                 long long c, const CladeSeg *__restrict__ seg,
                                                                 const CladeTile *__restrict__ tile, CladePiece *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long kb = off + (((long long)blockIdx.x * (kCladeThreads / 64) + (threadIdx.x >> 6)) << kCladeTileShift);
    if (kb >= off + c) return;      // (wave-uniform; no workgroup barrier below)
    const long long ke = min(kb + (1LL << kCladeTileShift), off + c);
    const long long t = kb >> kCladeTileShift;
    const CladeTile t0 = tile[t], t1 = tile[t + 1];
    const int np = t1.piece - t0.piece;
    for (int r = 0; r < np; r += 64) {
        const int j = r + lane;
        long long lo = 0, hi = 0;
        if (j < np) {
            lo = max(seg[t0.seg + j].first, kb);
            hi = min(seg[t0.seg + j + 1].first, ke);
        }
        const bool lane_piece = j < np && hi - lo <= kCladeLanePiece;
        if (lane_piece) {
            const float cx = clade_shift(x[lo - off]), cy = clade_shift(y[lo - off]);
            CladeAcc a;
            for (long long i = lo; i < hi; i++) a.add(x[i - off], y[i - off], (double)cx, (double)cy);
            clade_store(out + t0.piece + j, a, cx, cy);
        }
        unsigned long long wide = __ballot(j < np && !lane_piece);
        while (wide) {
            const int b = __ffsll((long long)wide) - 1;
            wide &= wide - 1;
            const long long wlo = __shfl(lo, b), whi = __shfl(hi, b);
            const float cx = clade_shift(x[wlo - off]), cy = clade_shift(y[wlo - off]);
            CladeAcc a;
            for (long long i = wlo + lane; i < whi; i += 64) a.add(x[i - off], y[i - off], (double)cx, (double)cy);
            clade_wave_reduce(a);
            if (lane == 0) clade_store(out + t0.piece + r + b, a, cx, cy);
        }
    }
}

}  // namespace st
