// kernels_rows.h -- included by suchtree_hip.hip (after kernels_clades.h).
// The reduction of st_compare_rows_host: row r's pairs sit at global indices r * S + k, k < P (SrcRows: S = P, or P
// rounded up to whole tiles with pairs [P, S) as padding).  A block is the row's pairs [2^kCladeTileShift b,
// min(2^kCladeTileShift (b + 1), P)), counted from the row's first pair; global block t is block t % nb of row t / nb
// (nb blocks per row), and chunks hold whole blocks.  This kernel writes one CladePiece per block and skips the padding;
// the host folds a row's blocks in block order (RowsReduce::drain, host_compare.h; clade_merge, compare_plan.cpp).
//
// Determinism: a block is summed about its own first pair in the order rule of k_clade_pieces, which depends on its
// length alone -- up to kCladeLanePiece pairs by one lane in index order, longer ones by one wave (lane l takes pairs l,
// l + 64, ... in order, then an xor butterfly, lane 0's result).  So a block's piece depends on its row's ids and the two
// trees only: not on the row's index, the other rows, the chunk or the grid.  No float atomics.
#pragma once

namespace st {

// One chunk: blocks [t0, t0 + n) of distances x / y[0 ..), whose index 0 is global pair `off`; out[j] receives block
// t0 + j.  Rows of at most kCladeLanePiece pairs (one block each) take one lane per block; otherwise one wave takes one
// block, and a short last block of a row is summed by its lane 0.
__global__ __launch_bounds__(kCladeThreads) void k_row_blocks(const float *__restrict__ x, const float *__restrict__ y, long long off,
                                                              long long S, long long P, long long nb, long long t0, long long n,
                                                              CladePiece *__restrict__ out)
{
    if (P <= kCladeLanePiece) {      // (then nb == 1 and S == P)
        const long long j = (long long)blockIdx.x * kCladeThreads + threadIdx.x;
        if (j >= n) return;
        const long long lo = (t0 + j) * S - off;
        const float cx = clade_shift(x[lo]), cy = clade_shift(y[lo]);
        CladeAcc a;
        for (long long i = lo; i < lo + P; i++) a.add(x[i], y[i], (double)cx, (double)cy);
        clade_store(out + j, a, cx, cy);
        return;
    }
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (kCladeThreads / 64) + (threadIdx.x >> 6);
    if (w >= n) return;      // (wave-uniform; no workgroup barrier below)
    const long long t = t0 + w, r = t / nb, b = t - r * nb;
    const long long lo = r * S + (b << kCladeTileShift) - off;
    const long long hi = r * S + min((b + 1) << kCladeTileShift, P) - off;
    const float cx = clade_shift(x[lo]), cy = clade_shift(y[lo]);
    CladeAcc a;
    if (hi - lo <= kCladeLanePiece) {
        if (lane == 0) {
            for (long long i = lo; i < hi; i++) a.add(x[i], y[i], (double)cx, (double)cy);
            clade_store(out + w, a, cx, cy);
        }
        return;
    }
    for (long long i = lo + lane; i < hi; i += 64) a.add(x[i], y[i], (double)cx, (double)cy);
    clade_wave_reduce(a);
    if (lane == 0) clade_store(out + w, a, cx, cy);
}

}  // namespace st
