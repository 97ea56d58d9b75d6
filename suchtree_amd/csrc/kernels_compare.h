// kernels_compare.h -- included by suchtree_hip.hip (after device_common.h).
// The reduction of the compare path (st_compare_triangle_host / st_compare_pairs_host): pair k has a float32 distance
// x[k] in tree X and y[k] in tree Y, written by the unchanged distance kernels into two device scratch chunks; these
// kernels reduce the chunks to the moments of the joint distribution and, if asked, an exact 2-D histogram.  Nothing
// is returned per pair.
//
// Determinism: every sum has one fixed order.  A lane sums its grid-stride share of a chunk in index order, a wave folds
// its lanes with xor shuffles, a workgroup folds its four waves in wave order and adds the result to ITS OWN partial
// slot (chunks run one after another on one stream, so slot b is only ever touched by workgroup b), and a final
// single-lane pass folds the slots in index order.  The grid is kCmpBlocks workgroups whatever the device or the chunk,
// so two identical calls return the same bits.  Histogram counts are integers: the order of their atomic adds does not
// change the result.
#pragma once

namespace st {

constexpr int kCmpBlocks = 1024;        // workgroups of k_pair_moments (fixed: the summation order depends on it)
constexpr int kCmpThreads = 256;        // lanes per workgroup (four waves)
constexpr int kCmpShiftPairs = 4096;    // the shift (cx, cy) is the mean of at most this many leading pairs
constexpr int kCmpMaxCells = 16384;     // histogram cells (uint32 counters in LDS: 64 KiB)

// one workgroup's running sums (and the final result): sums of (x - cx), (y - cy), their squares and cross product
struct CmpPartial {
    double sx, sy, sxx, syy, sxy;
    double min_x, max_x, min_y, max_y;   // NaN-ignoring (fmin / fmax); +inf / -inf when nothing was seen
    double pad;
};

struct CmpHist {
    const double *edges_x, *edges_y;   // bins_x + 1 and bins_y + 1 non-decreasing edges (device memory)
    int bins_x, bins_y;
    int edges_in_lds;                  // 1 = the kernel copies the edges to LDS behind the counters
    unsigned long long *out;           // (bins_x, bins_y) int64 counts, C order
};

// shift = mean of the first n (<= kCmpShiftPairs) pairs of the call, one workgroup; a non-finite mean (NaN or inf in
// that sample) is replaced by 0 so that the sums below stay finite wherever the data are
__global__ __launch_bounds__(kCmpThreads) void k_pair_shift(const float *__restrict__ x, const float *__restrict__ y, int n,
                                                             double *__restrict__ shift)
{
    __shared__ double sx_w[kCmpThreads / 64], sy_w[kCmpThreads / 64];
    double sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < n; i += kCmpThreads) {
        sx += (double)x[i];
        sy += (double)y[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sx += __shfl_xor(sx, off);
        sy += __shfl_xor(sy, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sx_w[threadIdx.x >> 6] = sx;
        sy_w[threadIdx.x >> 6] = sy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < kCmpThreads / 64; w++) {
            a += sx_w[w];
            b += sy_w[w];
        }
        a = n > 0 ? a / (double)n : 0.0;
        b = n > 0 ? b / (double)n : 0.0;
        shift[0] = isfinite(a) ? a : 0.0;
        shift[1] = isfinite(b) ? b : 0.0;
    }
}

// numpy.histogram2d's bin of v: searchsorted(edges, v, side='right') - 1, v == last edge in the last bin; -1 outside
// [edges[0], edges[bins]] and for NaN.  Binary search for the largest i in [0, bins) with edges[i] <= v.
__device__ __forceinline__ int cmp_bin(const double *e, int bins, double v)
{
    if (!(v >= e[0] && v <= e[bins])) return -1;
    int lo = 0, hi = bins;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct CmpLane {
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    double min_x = __builtin_huge_val(), max_x = -__builtin_huge_val();
    double min_y = __builtin_huge_val(), max_y = -__builtin_huge_val();

    __device__ __forceinline__ void add(float xf, float yf, double cx, double cy)
    {
        const double xv = (double)xf, yv = (double)yf;
        const double dx = xv - cx, dy = yv - cy;
        sx += dx;
        sy += dy;
        sxx += dx * dx;
        syy += dy * dy;
        sxy += dx * dy;
        min_x = fmin(min_x, xv);
        max_x = fmax(max_x, xv);
        min_y = fmin(min_y, yv);
        max_y = fmax(max_y, yv);
    }
};

// One chunk: x[0..n), y[0..n).  Lane t of the grid takes quads q = t, t + G*256, ... (four pairs, two 16-byte loads),
// then the n % 4 tail pairs go to the first lanes of the grid.  `first` (the call's first chunk) writes the slots
// instead of adding to them.  HIST: the same pairs are also binned into workgroup-private uint32 counters in LDS
// (a workgroup sees at most 2^25 / kCmpBlocks pairs per chunk: no overflow), added into the int64 histogram at the end.
template <bool HIST>
__global__ __launch_bounds__(kCmpThreads) void k_pair_moments(const float *__restrict__ x, const float *__restrict__ y, long long n,
                                                               const double *__restrict__ shift, int first,
                                                               CmpPartial *__restrict__ part, CmpHist hist)
{
    extern __shared__ unsigned cmp_lds[];
    __shared__ CmpPartial wave_part[kCmpThreads / 64];
    const double cx = shift[0], cy = shift[1];
    const int cells = HIST ? hist.bins_x * hist.bins_y : 0;
    const double *ex = hist.edges_x, *ey = hist.edges_y;
    if (HIST) {
        for (int c = threadIdx.x; c < cells; c += kCmpThreads) cmp_lds[c] = 0u;
        if (hist.edges_in_lds) {
            double *le = reinterpret_cast<double *>(cmp_lds + ((cells + 1) & ~1));
            for (int i = threadIdx.x; i <= hist.bins_x; i += kCmpThreads) le[i] = hist.edges_x[i];
            for (int i = threadIdx.x; i <= hist.bins_y; i += kCmpThreads) le[hist.bins_x + 1 + i] = hist.edges_y[i];
            ex = le;
            ey = le + hist.bins_x + 1;
        }
        __syncthreads();
    }
    CmpLane acc;
    auto bin = [&](float xf, float yf) {
        const int bx = cmp_bin(ex, hist.bins_x, (double)xf);
        const int by = cmp_bin(ey, hist.bins_y, (double)yf);
        if (bx >= 0 && by >= 0) atomicAdd(&cmp_lds[bx * hist.bins_y + by], 1u);
    };
    const long long lanes = (long long)gridDim.x * kCmpThreads;
    const long long lane = (long long)blockIdx.x * kCmpThreads + threadIdx.x;
    const long long quads = n >> 2;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    const float4 *y4 = reinterpret_cast<const float4 *>(y);
    for (long long q = lane; q < quads; q += lanes) {
        const float4 a = x4[q], b = y4[q];
        acc.add(a.x, b.x, cx, cy);
        acc.add(a.y, b.y, cx, cy);
        acc.add(a.z, b.z, cx, cy);
        acc.add(a.w, b.w, cx, cy);
        if (HIST) {
            bin(a.x, b.x);
            bin(a.y, b.y);
            bin(a.z, b.z);
            bin(a.w, b.w);
        }
    }
    if (lane < (n & 3)) {
        const long long i = (quads << 2) + lane;
        acc.add(x[i], y[i], cx, cy);
        if (HIST) bin(x[i], y[i]);
    }
    // wave fold (xor butterfly), then the four waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.sx += __shfl_xor(acc.sx, off);
        acc.sy += __shfl_xor(acc.sy, off);
        acc.sxx += __shfl_xor(acc.sxx, off);
        acc.syy += __shfl_xor(acc.syy, off);
        acc.sxy += __shfl_xor(acc.sxy, off);
        acc.min_x = fmin(acc.min_x, __shfl_xor(acc.min_x, off));
        acc.max_x = fmax(acc.max_x, __shfl_xor(acc.max_x, off));
        acc.min_y = fmin(acc.min_y, __shfl_xor(acc.min_y, off));
        acc.max_y = fmax(acc.max_y, __shfl_xor(acc.max_y, off));
    }
    if ((threadIdx.x & 63) == 0)
        wave_part[threadIdx.x >> 6] = CmpPartial{acc.sx, acc.sy, acc.sxx, acc.syy, acc.sxy, acc.min_x, acc.max_x, acc.min_y, acc.max_y, 0.0};
    __syncthreads();
    if (threadIdx.x == 0) {
        CmpPartial p = first ? CmpPartial{0.0, 0.0, 0.0, 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val(),
                                          __builtin_huge_val(), -__builtin_huge_val(), 0.0}
                             : part[blockIdx.x];
        for (int w = 0; w < kCmpThreads / 64; w++) {
            const CmpPartial &q = wave_part[w];
            p.sx += q.sx;
            p.sy += q.sy;
            p.sxx += q.sxx;
            p.syy += q.syy;
            p.sxy += q.sxy;
            p.min_x = fmin(p.min_x, q.min_x);
            p.max_x = fmax(p.max_x, q.max_x);
            p.min_y = fmin(p.min_y, q.min_y);
            p.max_y = fmax(p.max_y, q.max_y);
        }
        part[blockIdx.x] = p;
    }
    if (HIST) {      // (the __syncthreads above also ordered every LDS counter add before these reads)
        for (int c = threadIdx.x; c < cells; c += kCmpThreads) {
            const unsigned v = cmp_lds[c];
            if (v) atomicAdd(&hist.out[c], (unsigned long long)v);
        }
    }
}

// the kCmpBlocks slots in index order, one lane
__global__ __launch_bounds__(64) void k_pair_moments_final(const CmpPartial *__restrict__ part, int slots, CmpPartial *__restrict__ out)
{
    if (threadIdx.x != 0) return;
    CmpPartial p = part[0];
    for (int b = 1; b < slots; b++) {
        const CmpPartial &q = part[b];
        p.sx += q.sx;
        p.sy += q.sy;
        p.sxx += q.sxx;
        p.syy += q.syy;
        p.sxy += q.sxy;
        p.min_x = fmin(p.min_x, q.min_x);
        p.max_x = fmax(p.max_x, q.max_x);
        p.min_y = fmin(p.min_y, q.min_y);
        p.max_y = fmax(p.max_y, q.max_y);
    }
    *out = p;
}

}  // namespace st
