// host_compare.h -- part of suchtree_hip.hip (included after host_upload.h).  The device side of the compare paths
// (st_compare_*_host): compare_run drives chunks of pairs through the unchanged distance kernels of tree X and then
// tree Y into two float32 scratch buffers on the device, and a reducer -- MomentsReduce (kernels_compare.h), CladeReduce
// (kernels_clades.h), RowsReduce (kernels_rows.h) -- reduces them.  Device scratch is bounded by the chunk, host memory
// by the histogram or the pieces: nothing grows with the pair count.  What needs no GPU -- the clade plan and its
// tables, the rows layout, the folding of pieces -- is compare_plan.cpp.  The exact Spearman rank sums (compare_ranks)
// are three such runs around count tables that the entry point owns (kernels_ranks.h, rank_plan.cpp); the exact Kendall
// counts (compare_kendall) are one run that keeps every pair's key, then a sort (kernels_kendall.h, kendall_plan.cpp).
// The entry points st_compare_{triangle,pairs}[_ranks|_kendall]_host are one skeleton, compare_entry (at the end), over
// a pair input (TriangleInput, PairsInput, after compare_run) and a statistic (MomentsStat, RanksStat, KendallStat).
#pragma once

constexpr int64_t kCompareChunkTriangle = (int64_t)1 << 25;   // 2 x 128 MiB of float32 distances
constexpr int64_t kCompareChunkPairs = (int64_t)1 << 22;      // + 2 x 64 MiB of uploaded int64 pairs

// parts of one device block start on 256-byte boundaries
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// a kernel that sorts with perm_sort_lds is about to get `lds` bytes (perm_lds_bytes): above 32 KiB they are asked for
template <typename Kernel>
static hipError_t perm_lds_opt_in(Kernel *kernel, size_t lds)
{
    return lds <= 32 * 1024 ? hipSuccess : hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// The moments / 2-D histogram reduction of st_compare_triangle_host / st_compare_pairs_host (kernels_compare.h), as a
// reducer of compare_run: bytes(chunk) device bytes of its own, start() once, chunk() per chunk of distances, finish()
// enqueues the read-back, done() fills the result once the stream has drained.
struct MomentsReduce {
    const double *edges_x, *edges_y;
    int32_t bins_x, bins_y;
    st_pair_moments *out;
    int64_t *out_hist;
    int64_t count = 0;
    bool want_hist = false;
    int cells = 0, n_edges = 0;
    size_t o_final = 0, o_shift = 0, o_edges = 0, o_hist = 0, lds = 0;
    CmpPartial *d_part = nullptr, *d_final = nullptr;
    double *d_shift = nullptr;
    CmpHist H{};
    CmpPartial fin{};
    double shift[2] = {0.0, 0.0};

    size_t bytes(int64_t)
    {
        want_hist = out_hist != nullptr;
        cells = want_hist ? bins_x * bins_y : 0;
        n_edges = want_hist ? bins_x + bins_y + 2 : 0;
        o_final = align256(sizeof(CmpPartial) * kCmpBlocks);
        o_shift = o_final + align256(sizeof(CmpPartial));
        o_edges = o_shift + align256(16);
        o_hist = o_edges + align256((size_t)n_edges * 8);
        return o_hist + align256((size_t)cells * 8);
    }
    hipError_t start(char *d, int64_t total, hipStream_t s)
    {
        count = total;
        d_part = reinterpret_cast<CmpPartial *>(d);
        d_final = reinterpret_cast<CmpPartial *>(d + o_final);
        d_shift = reinterpret_cast<double *>(d + o_shift);
        double *d_edges = reinterpret_cast<double *>(d + o_edges);
        H = CmpHist{d_edges, d_edges + (want_hist ? bins_x + 1 : 0), bins_x, bins_y, 0, reinterpret_cast<unsigned long long *>(d + o_hist)};
        hipError_t e = hipSuccess;
        if (want_hist) {
            lds = (size_t)((cells + 1) & ~1) * 4;
            if (lds + (size_t)n_edges * 8 <= 128 * 1024) {      // edges beside the counters; else the kernel reads them from HBM (L2)
                lds += (size_t)n_edges * 8;
                H.edges_in_lds = 1;
            }
            e = hipMemcpyAsync(d_edges, edges_x, (size_t)(bins_x + 1) * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_edges + bins_x + 1, edges_y, (size_t)(bins_y + 1) * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemsetAsync(H.out, 0, (size_t)cells * 8, s);
            if (e == hipSuccess && lds > 64 * 1024 - 1024)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_pair_moments<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }
        return e;
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        if (off == 0)
            hipLaunchKernelGGL(k_pair_shift, dim3(1), dim3(kCmpThreads), 0, s, d_x, d_y, (int)std::min<int64_t>(c, kCmpShiftPairs), d_shift);
        if (want_hist)
            hipLaunchKernelGGL(k_pair_moments<true>, dim3(kCmpBlocks), dim3(kCmpThreads), lds, s, d_x, d_y, (long long)c, d_shift,
                               off == 0 ? 1 : 0, d_part, H);
        else
            hipLaunchKernelGGL(k_pair_moments<false>, dim3(kCmpBlocks), dim3(kCmpThreads), 0, s, d_x, d_y, (long long)c, d_shift,
                               off == 0 ? 1 : 0, d_part, H);
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        hipLaunchKernelGGL(k_pair_moments_final, dim3(1), dim3(64), 0, s, d_part, kCmpBlocks, d_final);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&fin, d_final, sizeof fin, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(shift, d_shift, sizeof shift, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && want_hist) e = hipMemcpyAsync(out_hist, H.out, (size_t)cells * 8, hipMemcpyDeviceToHost, s);
        return e;
    }
    int done()
    {
        *out = st_pair_moments{count, shift[0], shift[1], fin.sx, fin.sy, fin.sxx, fin.syy, fin.sxy, fin.min_x, fin.max_x, fin.min_y, fin.max_y};
        return ST_OK;
    }
};

// What the chunk drivers (compare_run below, quartet_run, hommola_clades_run, record_tree_run, unifrac_tree_depths) share: both trees'
// pipe mutexes, one device block, one stream, the two host fault words.  Declared after ST_DEVICE(...) and after whatever
// else its stream's work touches (device_res.h).  Both trees live on one device and so share its staging pipe and that
// pipe's mutex (host_tree.h): one lock, also when tree_x == tree_y; distinct mutexes (not possible today) are taken in
// address order.  `what` words the messages ("compare", "quartet compare").
struct TwoTreeSession {
    st_tree *tx, *ty;
    const char *what;
    std::unique_lock<std::mutex> lock_a, lock_b;
    DevBuf<char> d;
    DrainedStream s;

    TwoTreeSession(st_tree *x, st_tree *y, const char *w) : tx(x), ty(y), what(w)
    {
        std::mutex *ma = &tx->dp->m, *mb = &ty->dp->m;
        if (mb < ma) std::swap(ma, mb);
        lock_a = std::unique_lock<std::mutex>(*ma);
        if (mb != ma) lock_b = std::unique_lock<std::mutex>(*mb);
    }
    int hip_fail(const char *step, hipError_t e) const { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); }
    // the stream and the block of `total` bytes
    int open(size_t total)
    {
        hipError_t e = s.create();
        if (e == hipSuccess) e = d.alloc(total);
        return e == hipSuccess ? ST_OK : hip_fail(" setup: ", e);
    }
    // the same where the block is what a call may fail to get: ST_ERR_NOMEM, "<what>: <noun> of <total> bytes<detail>: ..."
    int open_or_nomem(size_t total, const char *noun, const std::string &detail = "")
    {
        hipError_t e = s.create();
        if (e != hipSuccess) return hip_fail(" setup: ", e);
        e = d.alloc(total);
        if (e == hipSuccess) return ST_OK;
        (void)hipGetLastError();
        return fail(ST_ERR_NOMEM, std::string(what) + ": " + noun + " of " + std::to_string(total) + " bytes" + detail + ": " + hipGetErrorString(e));
    }
    // arms both fault words (behind what the caller has staged on the stream) ...
    int arm() { return begin_host_faults(tx, s) != ST_OK || (ty != tx && begin_host_faults(ty, s) != ST_OK) ? ST_ERR_HIP : ST_OK; }
    // ... and reads them back once the stream has drained: tree X's fault is reported first
    int close(int64_t *bad_id)
    {
        Fault fx = kFaultInit, fy = kFaultInit;
        int rc = end_host_faults(tx, s, fx);
        if (rc == ST_OK && ty != tx) rc = end_host_faults(ty, s, fy);
        if (rc == ST_OK) rc = report_fault(tx->n_nodes, fx, bad_id);      // (not expected: the ids were checked on the host)
        if (rc == ST_OK) rc = report_fault(ty->n_nodes, fy, bad_id);
        return rc;
    }
};

// The two-slot read-back of a chunk driver whose host folds one chunk's results while the device works on the next: two
// pinned buffers of T, an event each, and what the caller has to know about a fill (Tag).  Per chunk: acquire() before
// the chunk's launches hands the fill of two chunks ago to `use`, the launches write the device twin of slot `next` (a
// part of the caller's block), post() copies it out.  flush() at the end hands over what is left, the older fill first:
// where results are merged, that order is part of their bits.  Declared before the session or stream that fills it.
template <typename T, typename Tag>
struct ReadbackRing {
    PinnedBuf<T> h[2];
    Event ev[2];
    Tag tag[2] = {};
    bool full[2] = {false, false};
    int next = 0;

    // both buffers (`count` elements each), then both events: after a failure, a null buffer tells which it was
    hipError_t alloc(size_t count)
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = h[i].alloc(count, hipHostMallocDefault);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = ev[i].create(hipEventDisableTiming);
        return e;
    }
    // the same as the status of the call `what`: a failed pinned buffer is ST_ERR_NOMEM with the bytes asked for, an event ST_ERR_HIP
    int alloc(size_t count, const char *what)
    {
        const hipError_t e = alloc(count);
        if (e == hipSuccess) return ST_OK;
        if (h[0] && h[1]) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
        (void)hipGetLastError();
        return fail(ST_ERR_NOMEM, std::string(what) + ": a pinned buffer of " + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    }
    template <typename Use>
    hipError_t acquire(Use use)
    {
        if (!full[next]) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ev[next]);
        if (e != hipSuccess) return e;
        use(h[next].get(), tag[next]);
        full[next] = false;
        return hipSuccess;
    }
    hipError_t post(const T *d_src, size_t n, const Tag &t, hipStream_t s)
    {
        hipError_t e = hipMemcpyAsync(h[next], d_src, n * sizeof(T), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev[next], s);
        if (e != hipSuccess) return e;
        tag[next] = t;
        full[next] = true;
        next ^= 1;
        return hipSuccess;
    }
    template <typename Use>
    hipError_t flush(Use use)
    {
        const hipError_t e = acquire(use);      // (`next` is the older slot)
        next ^= 1;
        return e == hipSuccess ? acquire(use) : e;
    }
    // the tail of a chunk loop: flush(), then the stream drained
    template <typename Use>
    hipError_t drain(Use use, hipStream_t s) { const hipError_t e = flush(use); return e == hipSuccess ? hipStreamSynchronize(s) : e; }
};

// A work block of `total` bytes and the ring, of `count` elements a slot, that reads its results back, for the call `what`:
// ST_OK, ST_ERR_NOMEM with the bytes asked for (the block, a pinned buffer) or ST_ERR_HIP (an event).
template <typename T, typename Tag>
static int alloc_work(DevBuf<char> &d, size_t total, ReadbackRing<T, Tag> &ring, size_t count, const char *what)
{
    const hipError_t e = d.alloc(total);
    if (e == hipSuccess) return ring.alloc(count, what);
    (void)hipGetLastError();
    return fail(ST_ERR_NOMEM, std::string(what) + ": a work block of " + std::to_string(total) + " bytes: " + hipGetErrorString(e));
}

struct BlockSpan {      // the tag of a slot of pieces: global blocks [first, first + count)
    int64_t first, count;
};

// count pairs in chunks of `chunk`: prep(stream, off, c) stages what chunk [off, off + c) needs, src_x(off) / src_y(off)
// are its pair sources in tree X / Y, `red` reduces the two chunks of distances (MomentsReduce, CladeReduce).  `extra`
// device bytes are handed to `setup` once (the caller's ids or pairs).
template <typename Setup, typename Prep, typename SrcX, typename SrcY, typename Reduce>
static int compare_run(st_tree *tx, st_tree *ty, int64_t count, int64_t chunk, size_t extra, Setup setup, Prep prep, SrcX src_x,
                       SrcY src_y, Reduce &red, int64_t *bad_id)
{
    ST_DEVICE(tx->device);
    TwoTreeSession ses(tx, ty, "compare");
    chunk = std::min(chunk, count);
    // one device block: x | y | the reducer's | caller's data
    const size_t o_y = align256((size_t)chunk * 4), o_red = o_y + align256((size_t)chunk * 4);
    const size_t o_extra = o_red + align256(red.bytes(chunk)), total = o_extra + align256(extra);
    int rc = ses.open(total);
    if (rc != ST_OK) return rc;
    char *const d = ses.d;
    const hipStream_t s = ses.s;
    float *d_x = reinterpret_cast<float *>(d), *d_y = reinterpret_cast<float *>(d + o_y);
    char *d_extra = d + o_extra;
    hipError_t e = red.start(d + o_red, count, s);
    if (e == hipSuccess) e = setup(d_extra, s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    rc = ses.arm();
    if (rc != ST_OK) return rc;
    for (int64_t off = 0; off < count; off += chunk) {
        const int64_t c = std::min(chunk, count - off);
        e = prep(d_extra, s, off, c);
        if (e != hipSuccess) return ses.hip_fail(" upload: ", e);
        rc = enqueue_src(tx, src_x(d_extra, off), c, DistSink{nullptr, d_x}, MrcaSink{nullptr, nullptr}, tx->d_fault_host, s);
        if (rc == ST_OK)
            rc = enqueue_src(ty, src_y(d_extra, off), c, DistSink{nullptr, d_y}, MrcaSink{nullptr, nullptr}, ty->d_fault_host, s);
        if (rc != ST_OK) return rc;
        e = red.chunk(d_x, d_y, off, c, s);
        if (e != hipSuccess) return ses.hip_fail(" launch: ", e);
    }
    e = red.finish(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    rc = ses.close(bad_id);
    if (rc != ST_OK) return rc;
    return red.done();
}

// ---- the two pair inputs of compare_entry (at the end): what the caller's pairs are, how they are checked and how one
// compare_run goes over them.  A new pair source is one more such struct.
static int triangle_range_args(int64_t m, int64_t k_begin, int64_t k_count)      // (st_triangle_* check their range with it too)
{
    if (m < 0 || k_begin < 0 || k_count < 0) return fail(ST_ERR_ARG, "negative size");
    if (m > 3000000000LL) return fail(ST_ERR_ARG, "m too large");
    if (k_begin + k_count > m * (m - 1) / 2) return fail(ST_ERR_ARG, "pair range exceeds m(m-1)/2");
    return ST_OK;
}

// ids on the host, before anything is launched: ST_ERR_BOUNDS with the id the reference reports (MuchTree.pyx:897-903)
static int compare_check_ids(const int64_t *ids, int64_t n, int64_t n_nodes, int64_t *bad_id)
{
    Fault f = kFaultInit;
    ids_in_range(ids, n, n_nodes, f.max_bad, f.min_bad);
    return report_fault(n_nodes, f, bad_id);
}

// n ids of tree X, then n of tree Y
static int compare_check_ids(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t n, int64_t *bad_id)
{
    const int rc = compare_check_ids(ids_x, n, tx->n_nodes, bad_id);
    return rc != ST_OK ? rc : compare_check_ids(ids_y, n, ty->n_nodes, bad_id);
}

// pairs [k_begin, k_begin + k_count) of the triangle over two aligned id lists; chunk_pairs 0: the path's default chunk
struct TriangleInput {
    const int64_t *ids_x, *ids_y;
    int64_t m, k_begin, k_count;

    int64_t count() const { return k_count; }
    int range_args() const { return triangle_range_args(m, k_begin, k_count); }
    int null_args() const { return m > 0 && (!ids_x || !ids_y) ? fail(ST_ERR_ARG, "ids_x or ids_y is NULL") : ST_OK; }
    int check_ids(st_tree *tx, st_tree *ty, int64_t *bad_id) const { return compare_check_ids(tx, ty, ids_x, ids_y, m, bad_id); }
    template <typename Reduce>
    int run(st_tree *tx, st_tree *ty, int64_t chunk_pairs, Reduce &red, int64_t *bad_id) const
    {
        auto setup = [&](char *d_extra, hipStream_t s) {
            hipError_t e = hipMemcpyAsync(d_extra, ids_x, (size_t)m * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_extra + (size_t)m * 8, ids_y, (size_t)m * 8, hipMemcpyHostToDevice, s);
            return e;
        };
        auto prep = [](char *, hipStream_t, int64_t, int64_t) { return hipSuccess; };
        auto src_x = [&](char *d_extra, int64_t off) {
            return SrcTriangle{reinterpret_cast<const long long *>(d_extra), 1, (long long)(k_begin + off)};
        };
        auto src_y = [&](char *d_extra, int64_t off) {
            return SrcTriangle{reinterpret_cast<const long long *>(d_extra) + m, 1, (long long)(k_begin + off)};
        };
        return compare_run(tx, ty, k_count, chunk_pairs > 0 ? chunk_pairs : kCompareChunkTriangle, (size_t)m * 16, setup, prep, src_x, src_y,
                           red, bad_id);
    }
};

// n explicit pairs, row i of pairs_x in tree X against row i of pairs_y in tree Y, uploaded chunk by chunk
struct PairsInput {
    const int64_t *pairs_x, *pairs_y;
    int64_t n;

    int64_t count() const { return n; }
    int range_args() const { return n < 0 ? fail(ST_ERR_ARG, "n < 0") : ST_OK; }
    int null_args() const { return n > 0 && (!pairs_x || !pairs_y) ? fail(ST_ERR_ARG, "pairs_x or pairs_y is NULL") : ST_OK; }
    int check_ids(st_tree *tx, st_tree *ty, int64_t *bad_id) const { return compare_check_ids(tx, ty, pairs_x, pairs_y, 2 * n, bad_id); }
    template <typename Reduce>
    int run(st_tree *tx, st_tree *ty, int64_t chunk_pairs, Reduce &red, int64_t *bad_id) const
    {
        const int64_t chunk = std::min(n, chunk_pairs > 0 ? chunk_pairs : kCompareChunkPairs);
        auto setup = [](char *, hipStream_t) { return hipSuccess; };
        auto prep = [&](char *d_extra, hipStream_t s, int64_t off, int64_t c) {
            hipError_t e = hipMemcpyAsync(d_extra, pairs_x + 2 * off, (size_t)c * 16, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_extra + (size_t)chunk * 16, pairs_y + 2 * off, (size_t)c * 16, hipMemcpyHostToDevice, s);
            return e;
        };
        auto src_x = [](char *d_extra, int64_t) { return SrcContig{reinterpret_cast<const long long *>(d_extra)}; };
        auto src_y = [&](char *d_extra, int64_t) { return SrcContig{reinterpret_cast<const long long *>(d_extra + (size_t)chunk * 16)}; };
        return compare_run(tx, ty, n, chunk, (size_t)chunk * 32, setup, prep, src_x, src_y, red, bad_id);
    }
};

// The reducer of st_compare_clades_host: k_clade_pieces per chunk into one device array of pieces, read back at the end;
// done() merges pieces into segments (index order) and segments into nodes (children first, in id order, then the
// node's own segments) on the host.
struct CladeReduce {
    const CladePlan &P;
    const CladeTables &T;
    st_pair_moments *out;
    int64_t cap;
    const CladeSeg *d_seg = nullptr;             // (set by the caller's setup)
    const CladeTile *d_tile = nullptr;
    CladePiece *d_pieces = nullptr;
    std::vector<CladePiece> pieces;

    size_t bytes(int64_t) { return (size_t)T.n_pieces * sizeof(CladePiece); }
    hipError_t start(char *d, int64_t, hipStream_t)
    {
        d_pieces = reinterpret_cast<CladePiece *>(d);
        return hipSuccess;
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        const int64_t tiles_c = (c + ST_CLADE_TILE - 1) / ST_CLADE_TILE;
        const int64_t blocks = (tiles_c + kCladeThreads / 64 - 1) / (kCladeThreads / 64);
        hipLaunchKernelGGL(k_clade_pieces, dim3((unsigned)blocks), dim3(kCladeThreads), 0, s, d_x, d_y, (long long)off, (long long)c, d_seg,
                           d_tile, d_pieces);
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        pieces.resize(T.n_pieces);
        return hipMemcpyAsync(pieces.data(), d_pieces, (size_t)T.n_pieces * sizeof(CladePiece), hipMemcpyDeviceToHost, s);
    }
    int done()
    {
        clade_fold(P, T, pieces.data(), cap, out);
        return ST_OK;
    }
};

// st_compare_clades_host behind its checks and its plan (red.P, red.T; at least one pair): the links staged in the plan's order, then
// the chunks of `chunk` pairs.
static int clades_run(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t n_links, int64_t chunk, CladeReduce &red,
                      int64_t *bad_id)
{
    const CladePlan &P = red.P;
    const CladeTables &T = red.T;
    // device: permuted ids of X and Y and ranks (int32) | segments | tiles
    const size_t L = (size_t)n_links;
    const size_t o_y = align256(L * 4), o_rank = o_y + align256(L * 4), o_seg = o_rank + align256(L * 4);
    const size_t o_tile = o_seg + align256(T.segs.size() * sizeof(CladeSeg)), extra = o_tile + align256(T.tiles.size() * sizeof(CladeTile));
    std::vector<int32_t> sx(L), sy(L), rk(L);
    for (size_t p = 0; p < L; p++) {
        const int64_t j = P.perm[p];
        sx[p] = (int32_t)ids_x[j];
        sy[p] = (int32_t)ids_y[j];
        rk[p] = (int32_t)j;
    }
    auto setup = [&](char *d, hipStream_t s) {
        red.d_seg = reinterpret_cast<const CladeSeg *>(d + o_seg);
        red.d_tile = reinterpret_cast<const CladeTile *>(d + o_tile);
        hipError_t e = hipMemcpyAsync(d, sx.data(), L * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_y, sy.data(), L * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_rank, rk.data(), L * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_seg, T.segs.data(), T.segs.size() * sizeof(CladeSeg), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_tile, T.tiles.data(), T.tiles.size() * sizeof(CladeTile), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the host vectors are pageable and go out of scope with this call)
        return e;
    };
    auto prep = [](char *, hipStream_t, int64_t, int64_t) { return hipSuccess; };
    auto src = [&](size_t o_ids) {
        return [&, o_ids](char *d, int64_t off) {
            return SrcSegments{reinterpret_cast<const int *>(d + o_ids), reinterpret_cast<const int *>(d + o_rank),
                               reinterpret_cast<const CladeSeg *>(d + o_seg), reinterpret_cast<const CladeTile *>(d + o_tile), (long long)off};
        };
    };
    return compare_run(tx, ty, P.total, chunk, extra, setup, prep, src(0), src(o_y), red, bad_id);
}

// The reducer of st_compare_rows_host: k_row_blocks per chunk into one of two device piece buffers, each read back into
// its pinned host twin (ReadbackRing); the host folds a chunk's pieces into their rows (block order, clade_merge) while
// the device works on the next chunk.  Pieces of at most two chunks exist at any time.
struct RowsReduce {
    const RowsLayout &L;
    st_pair_moments *out;
    CladePiece *d_pieces[2] = {nullptr, nullptr};      // (parts of compare_run's block)
    ReadbackRing<CladePiece, BlockSpan> ring;

    RowsReduce(const RowsLayout &l, st_pair_moments *o) : L(l), out(o) {}
    size_t piece_bytes() const { return align256((size_t)L.max_blocks * sizeof(CladePiece)); }
    size_t bytes(int64_t) { return 2 * piece_bytes(); }
    hipError_t start(char *d, int64_t, hipStream_t)
    {
        for (int i = 0; i < 2; i++) d_pieces[i] = reinterpret_cast<CladePiece *>(d + i * piece_bytes());
        return ring.alloc((size_t)L.max_blocks);
    }
    void fold(const CladePiece *pieces, const BlockSpan &b)
    {
        for (int64_t j = 0; j < b.count; j++) {
            const int64_t t = b.first + j;
            clade_merge(out[t / L.nb], piece_moments(pieces[j], L.block_len(t)));
        }
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        hipError_t e = ring.acquire([&](const CladePiece *p, const BlockSpan &b) { fold(p, b); });      // (the pieces of two chunks ago)
        if (e != hipSuccess) return e;
        const int64_t t0 = L.block_of(off), n = L.block_of(off + c - 1) + 1 - t0, tl = t0 + n - 1;
        if (n > L.max_blocks || L.block_lo(t0) != off || L.block_lo(tl) + L.block_len(tl) > off + c) return hipErrorInvalidValue;
        const int64_t per = L.P <= kCladeLanePiece ? kCladeThreads : kCladeThreads / 64;      // blocks per workgroup
        CladePiece *const d_out = d_pieces[ring.next];
        hipLaunchKernelGGL(k_row_blocks, dim3((unsigned)((n + per - 1) / per)), dim3(kCladeThreads), 0, s, d_x, d_y, (long long)off,
                           (long long)L.S, (long long)L.P, (long long)L.nb, (long long)t0, (long long)n, d_out);
        e = hipGetLastError();
        if (e == hipSuccess) e = ring.post(d_out, (size_t)n, BlockSpan{t0, n}, s);
        return e;
    }
    hipError_t finish(hipStream_t) { return hipSuccess; }
    int done()
    {
        const hipError_t e = ring.flush([&](const CladePiece *p, const BlockSpan &b) { fold(p, b); });
        return e == hipSuccess ? ST_OK : fail(ST_ERR_HIP, std::string("rows read-back: ") + hipGetErrorString(e));
    }
};

// st_compare_rows_host behind its checks: n_rows > 0 rows of m checked ids each (below n_nodes, so int32), staged and run.
static int rows_run(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t n_rows, int64_t m, const RowsLayout &L,
                    st_pair_moments *out, int64_t *bad_id)
{
    const int64_t n_ids = n_rows * m;
    const std::vector<int32_t> hx(ids_x, ids_x + n_ids), hy(ids_y, ids_y + n_ids);
    // device: the int32 ids of up to max_rows rows from row `up_lo` on, X then Y; uploaded again when a chunk needs others
    const size_t row_bytes = (size_t)m * 4, half = align256((size_t)L.max_rows * row_bytes);
    int64_t up_lo = -1, up_hi = -1;
    auto setup = [](char *, hipStream_t) { return hipSuccess; };
    auto prep = [&](char *d, hipStream_t s, int64_t off, int64_t c) {
        const int64_t r0 = off / L.S, r1 = (off + c - 1) / L.S + 1;
        if (r1 - r0 > L.max_rows) return hipErrorInvalidValue;
        if (r0 >= up_lo && r1 <= up_hi) return hipSuccess;
        up_lo = r0;
        up_hi = std::min(n_rows, r0 + L.max_rows);
        const size_t b = (size_t)(up_hi - up_lo) * row_bytes;
        hipError_t e = hipMemcpyAsync(d, hx.data() + up_lo * m, b, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + half, hy.data() + up_lo * m, b, hipMemcpyHostToDevice, s);
        return e;
    };
    auto src = [&](size_t o) {
        return [&, o](char *d, int64_t off) {
            return SrcRows{reinterpret_cast<const int *>(d + o), (long long)m, (long long)L.P, (long long)L.S, 1.0 / (double)L.S,
                           (long long)off, (long long)up_lo};
        };
    };
    RowsReduce red(L, out);
    return compare_run(tx, ty, n_rows * L.S, L.chunk, 2 * half, setup, prep, src(0), src(half), red, bad_id);
}

// ---- exact Spearman rank sums (st_compare_*_ranks_host; kernels_ranks.h, rank_plan.h) ------------------------------
// What the three passes share.  It outlives each pass's compare_run (which frees its own block), so the entry point
// owns it: its members free everything on every path out.
struct RankState {
    DevBuf<char> d_small;                    // occupancy | slots | miss | scan shares | scan results | dot slots | dot result
    DevBuf<unsigned> d_tab[2];                    // tree X's and tree Y's counters, then their a
    DevBuf<unsigned long long> d_block_sum;
    RankSlots slots[2];
    int h_slots[2 * kRankBuckets];
    RankOccupancy occ;
    RankScanPart scan[2];
    RankDotPart dot;
    unsigned miss = 0;
    int64_t n = 0;

    static constexpr size_t o_slots = (sizeof(RankOccupancy) + 255) & ~(size_t)255;
    static constexpr size_t o_miss = o_slots + sizeof(int) * 2 * kRankBuckets;
    static constexpr size_t o_parts = o_miss + 256;
    static constexpr size_t o_scan = o_parts + sizeof(RankScanPart) * kRankBlocks;
    static constexpr size_t o_dot = o_scan + 256;
    static constexpr size_t o_dot_final = o_dot + sizeof(RankDotPart) * kRankBlocks;
    static constexpr size_t small_bytes = o_dot_final + 256;

    RankOccupancy *d_occ() const { return reinterpret_cast<RankOccupancy *>(d_small.get()); }
    int *d_slots() const { return reinterpret_cast<int *>(d_small + o_slots); }
    unsigned *d_miss() const { return reinterpret_cast<unsigned *>(d_small + o_miss); }
    RankScanPart *d_parts() const { return reinterpret_cast<RankScanPart *>(d_small + o_parts); }
    RankScanPart *d_scan() const { return reinterpret_cast<RankScanPart *>(d_small + o_scan); }
    RankDotPart *d_dot() const { return reinterpret_cast<RankDotPart *>(d_small + o_dot); }
    RankDotPart *d_dot_final() const { return reinterpret_cast<RankDotPart *>(d_small + o_dot_final); }
    size_t tab_bytes(int t) const { return (size_t)slots[t].n_slots * (size_t)kRankBucketKeys * 4; }
    int64_t scan_blocks(int t) const { return (int64_t)slots[t].n_slots * (kRankBucketKeys / kRankScanBlock); }

    // between pass 0 and pass 1: the slots of the occupied buckets and the tables they need
    int tables()
    {
        for (int t = 0; t < 2; t++) {
            rank_slots(occ.occ + t * kRankBuckets, slots[t]);
            std::copy(slots[t].slot, slots[t].slot + kRankBuckets, h_slots + t * kRankBuckets);
            uint64_t seen = 0;
            for (int b = 0; b < kRankBuckets; b++) seen += occ.occ[t * kRankBuckets + b];
            if ((int64_t)seen != n) return fail(ST_ERR_HIP, "ranks: the occupancy pass saw " + std::to_string(seen) + " of " + std::to_string(n) + " values");
        }
        for (int t = 0; t < 2; t++) {
            const hipError_t e = d_tab[t].alloc(tab_bytes(t) / 4);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(ST_ERR_NOMEM, "ranks: the distances occupy " + std::to_string(slots[0].n_slots) + " + " + std::to_string(slots[1].n_slots) +
                                              " of " + std::to_string(kRankBuckets) + " key buckets, 4 MiB of counters each: " + hipGetErrorString(e));
            }
        }
        const hipError_t e = d_block_sum.alloc((size_t)std::max(scan_blocks(0), scan_blocks(1)));
        if (e != hipSuccess) return fail(ST_ERR_NOMEM, std::string("ranks: ") + hipGetErrorString(e));
        return ST_OK;
    }
    int missed(const char *pass) const
    {
        if (miss == 0) return ST_OK;
        return fail(ST_ERR_HIP, std::string("ranks: ") + std::to_string(miss) + " values of the " + pass + " pass fell in buckets the first pass had not seen");
    }
};

// pass 0: the moments of st_compare_*_host (the same kernels in the same order: the same bits) and the occupancy
struct RankOccupancyReduce {
    MomentsReduce mom;
    RankState &R;

    size_t bytes(int64_t c) { return mom.bytes(c); }
    hipError_t start(char *d, int64_t total, hipStream_t s)
    {
        hipError_t e = mom.start(d, total, s);
        if (e == hipSuccess) e = hipMemsetAsync(R.d_occ(), 0, sizeof(RankOccupancy), s);
        return e;
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        hipError_t e = mom.chunk(d_x, d_y, off, c, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rank_occupancy, dim3(kRankBlocks), dim3(kRankThreads), 0, s, d_x, d_y, (long long)c, R.d_occ());
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        hipError_t e = mom.finish(s);
        if (e == hipSuccess) e = hipMemcpyAsync(&R.occ, R.d_occ(), sizeof(RankOccupancy), hipMemcpyDeviceToHost, s);
        return e;
    }
    int done() { return mom.done(); }
};

// pass 1: count every value, then the scan of each table in key order
struct RankCountReduce {
    RankState &R;

    size_t bytes(int64_t) { return 0; }
    hipError_t start(char *, int64_t, hipStream_t s)
    {
        hipError_t e = hipMemcpyAsync(R.d_slots(), R.h_slots, sizeof R.h_slots, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(R.d_miss(), 0, 4, s);
        for (int t = 0; t < 2 && e == hipSuccess; t++) e = hipMemsetAsync(R.d_tab[t], 0, R.tab_bytes(t), s);
        return e;
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t, int64_t c, hipStream_t s)
    {
        hipLaunchKernelGGL(k_rank_count, dim3(kRankBlocks), dim3(kRankThreads), 0, s, d_x, d_y, (long long)c, R.d_slots(), R.d_tab[0],
                           R.d_tab[1], R.d_miss());
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        for (int t = 0; t < 2; t++) {
            const int64_t nb = R.scan_blocks(t);
            const int grid = (int)std::min<int64_t>(nb, kRankBlocks);
            hipLaunchKernelGGL(k_rank_block_sums, dim3(grid), dim3(kRankThreads), 0, s, R.d_tab[t], (long long)nb, R.d_block_sum, R.d_parts());
            hipLaunchKernelGGL(k_rank_scan_blocks, dim3(1), dim3(kRankThreads), 0, s, R.d_block_sum, (long long)nb, R.d_parts(), grid,
                               R.d_scan() + t);
            hipLaunchKernelGGL(k_rank_scan_apply, dim3((unsigned)nb), dim3(kRankThreads), 0, s, R.d_tab[t], R.d_block_sum, (long long)R.n);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipMemcpyAsync(R.scan, R.d_scan(), sizeof R.scan, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&R.miss, R.d_miss(), 4, hipMemcpyDeviceToHost, s);
        return e;
    }
    int done()
    {
        const int rc = R.missed("count");
        if (rc != ST_OK) return rc;
        for (int t = 0; t < 2; t++)
            if ((int64_t)R.scan[t].total != R.n) return fail(ST_ERR_HIP, "ranks: the scan counted " + std::to_string(R.scan[t].total) + " of " + std::to_string(R.n) + " values");
        return ST_OK;
    }
};

// pass 2: sum of a_x * a_y
struct RankDotReduce {
    RankState &R;

    size_t bytes(int64_t) { return 0; }
    hipError_t start(char *, int64_t, hipStream_t s) { return hipMemsetAsync(R.d_miss(), 0, 4, s); }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        hipLaunchKernelGGL(k_rank_dot, dim3(kRankBlocks), dim3(kRankThreads), 0, s, d_x, d_y, (long long)c, R.d_slots(),
                           reinterpret_cast<const int *>(R.d_tab[0].get()), reinterpret_cast<const int *>(R.d_tab[1].get()), off == 0 ? 1 : 0, R.d_dot(),
                           R.d_miss());
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        hipLaunchKernelGGL(k_rank_dot_final, dim3(1), dim3(64), 0, s, R.d_dot(), kRankBlocks, R.d_dot_final());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&R.dot, R.d_dot_final(), sizeof R.dot, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&R.miss, R.d_miss(), 4, hipMemcpyDeviceToHost, s);
        return e;
    }
    int done() { return R.missed("lookup"); }
};

// The three passes.  run(chunk_pairs, reducer) is one compare_run over the caller's pairs; chunk_pairs 0 = the path's
// default, which pass 0 always takes so that its moments are those of st_compare_*_host.
template <typename Run>
static int compare_ranks(st_tree *tx, int64_t n, int64_t chunk_pairs, Run run, st_pair_moments *out, st_rank_sums *out_ranks)
{
    ST_DEVICE(tx->device);
    auto R = std::make_unique<RankState>();
    R->n = n;
    const hipError_t e = R->d_small.alloc(RankState::small_bytes);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("ranks setup: ") + hipGetErrorString(e));
    RankOccupancyReduce occupancy{MomentsReduce{nullptr, nullptr, 0, 0, out, nullptr}, *R};
    int rc = run((int64_t)0, occupancy);
    if (rc != ST_OK) return rc;
    if (R->occ.n_nan > 0) {
        rank_finish(n, (int64_t)R->occ.n_nan, 0, 0, 0, 0, 0, out_ranks);
        return ST_OK;
    }
    rc = R->tables();
    if (rc != ST_OK) return rc;
    RankCountReduce count{*R};
    rc = run(chunk_pairs, count);
    if (rc != ST_OK) return rc;
    RankDotReduce dot{*R};
    rc = run(chunk_pairs, dot);
    if (rc != ST_OK) return rc;
    const i128 sxy = (i128)(((u128)(uint64_t)R->dot.hi << 64) | R->dot.lo);
    rank_finish(n, 0, (int64_t)R->scan[0].distinct, (int64_t)R->scan[1].distinct, sxy, ((u128)R->scan[0].tie_hi << 64) | R->scan[0].tie_lo,
                ((u128)R->scan[1].tie_hi << 64) | R->scan[1].tie_lo, out_ranks);
    return ST_OK;
}

// ---- exact Kendall tau-b counts (st_compare_*_kendall_host, st_kendall_arrays_host; kernels_kendall.h, kendall_plan.h) ----
// The pairs' keys and the sort's second buffer: 16 bytes per pair, which outlive the compare_run that fills them, so the
// entry point owns them.  The 32-bit stage lives inside the two buffers: after the 64-bit sort one holds the sorted keys
// and the other is spare -- it takes the block records of the two tie scans, then the low words in its first 4 n bytes
// with their sort's second buffer in the last 4 n; the buffer of the sorted keys is spare for the last tie scan.
struct KendallState {
    DevBuf<unsigned long long> d_keys[2];
    DevBuf<char> d_small;                    // NaN pairs | slots of the four counts | the four counts
    int64_t n = 0;
    unsigned long long counts[kKendallCounts] = {0, 0, 0, 0}, n_nan = 0;

    static constexpr size_t o_part = 256;
    static constexpr size_t o_final = o_part + sizeof(unsigned long long) * kKendallCounts * kKendallBlocks;
    static constexpr size_t small_bytes = o_final + 256;

    unsigned long long *d_nan() const { return reinterpret_cast<unsigned long long *>(d_small.get()); }
    unsigned long long *d_part(int count) const { return reinterpret_cast<unsigned long long *>(d_small + o_part) + (size_t)count * kKendallBlocks; }
    unsigned long long *d_final() const { return reinterpret_cast<unsigned long long *>(d_small + o_final); }

    // everything the call needs beside compare_run's block, or nothing
    int alloc(int64_t pairs)
    {
        n = pairs;
        const size_t bytes = (size_t)n * 8;
        hipError_t e = d_small.alloc(small_bytes);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = d_keys[i].alloc((size_t)n);
        if (e == hipSuccess) return ST_OK;
        (void)hipGetLastError();
        d_small.reset();
        d_keys[0].reset();
        d_keys[1].reset();
        return fail(ST_ERR_NOMEM, "Kendall counts of " + std::to_string(n) + " pairs need two device buffers of " + std::to_string(bytes) +
                                      " bytes each (16 bytes per pair) and " + std::to_string(small_bytes) + " more: " + hipGetErrorString(e));
    }
    hipError_t start(hipStream_t s) { return hipMemsetAsync(d_small, 0, small_bytes, s); }
    int grid() const { return (int)std::min<int64_t>((n + kKendallTile - 1) / kKendallTile, kKendallBlocks); }

    // src (n keys) sorted, ping-ponging with `other`; returns the buffer that holds the result
    template <typename Key, bool Count>
    Key *sort(Key *src, Key *other, hipStream_t s)
    {
        hipLaunchKernelGGL((k_kendall_tile_sort<Key, Count>), dim3(grid()), dim3(kKendallThreads), 0, s, src, src, (long long)n, d_part(kKendallDiscordant));
        for (int64_t run = kKendallTile; run < n; run <<= 1) {
            hipLaunchKernelGGL((k_kendall_merge<Key, Count>), dim3(grid()), dim3(kKendallThreads), 0, s, src, other, (long long)n, (long long)run,
                               d_part(kKendallDiscordant));
            std::swap(src, other);
        }
        return src;
    }
    // the tie sum of sorted[0, n) by (key >> shift) into the slots of `count`; `blocks`: room for one int per tile
    template <typename Key>
    void ties(const Key *sorted, int shift, int count, int *blocks, hipStream_t s)
    {
        const int64_t n_blocks = (n + kKendallTile - 1) / kKendallTile;
        hipLaunchKernelGGL(k_kendall_tie_blocks<Key>, dim3(grid()), dim3(kKendallThreads), 0, s, sorted, (long long)n, shift, blocks);
        hipLaunchKernelGGL(k_kendall_tie_carry, dim3(1), dim3(kKendallThreads), 0, s, blocks, (long long)n_blocks);
        hipLaunchKernelGGL(k_kendall_tie_sums<Key>, dim3(grid()), dim3(kKendallThreads), 0, s, sorted, (long long)n, shift, blocks, d_part(count));
    }
    // everything after the keys (in d_keys[0]), and the read-back; n >= 1
    hipError_t enqueue(hipStream_t s)
    {
        unsigned long long *sorted = sort<unsigned long long, false>(d_keys[0].get(), d_keys[1].get(), s);
        unsigned long long *spare = sorted == d_keys[0].get() ? d_keys[1].get() : d_keys[0].get();
        ties(sorted, 32, kKendallTiesX, reinterpret_cast<int *>(spare), s);
        ties(sorted, 0, kKendallTiesXY, reinterpret_cast<int *>(spare), s);
        uint32_t *low = reinterpret_cast<uint32_t *>(spare);
        hipLaunchKernelGGL(k_kendall_low_words, dim3(grid()), dim3(kKendallThreads), 0, s, sorted, (long long)n, low);
        const uint32_t *low_sorted = sort<uint32_t, true>(low, low + n, s);
        ties(low_sorted, 0, kKendallTiesY, reinterpret_cast<int *>(sorted), s);
        hipLaunchKernelGGL(k_kendall_final, dim3(kKendallCounts), dim3(64), 0, s, d_part(0), d_final());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(counts, d_final(), sizeof counts, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_nan, d_nan(), sizeof n_nan, hipMemcpyDeviceToHost, s);
        return e;
    }
    void done(st_kendall_counts *out) const
    {
        kendall_finish(n, (int64_t)n_nan, counts[kKendallDiscordant], counts[kKendallTiesX], counts[kKendallTiesY], counts[kKendallTiesXY], out);
    }
};

// The reducer of the Kendall path: every chunk's keys at the chunk's offset, the sort and the counts in finish().  With
// `moments` it also is the MomentsReduce of st_compare_*_host (the same kernels in the same order: the same bits).
struct KendallKeysReduce {
    MomentsReduce mom;
    KendallState &K;
    bool moments;

    size_t bytes(int64_t c) { return moments ? mom.bytes(c) : 0; }
    hipError_t start(char *d, int64_t total, hipStream_t s)
    {
        hipError_t e = moments ? mom.start(d, total, s) : hipSuccess;
        if (e == hipSuccess) e = K.start(s);
        return e;
    }
    hipError_t chunk(const float *d_x, const float *d_y, int64_t off, int64_t c, hipStream_t s)
    {
        hipError_t e = moments ? mom.chunk(d_x, d_y, off, c, s) : hipSuccess;
        if (e != hipSuccess) return e;
        const int grid = (int)std::min<int64_t>((c + kKendallThreads - 1) / kKendallThreads, kKendallBlocks);
        hipLaunchKernelGGL(k_kendall_keys, dim3(grid), dim3(kKendallThreads), 0, s, d_x, d_y, (long long)c, K.d_keys[0] + off, K.d_nan());
        return hipGetLastError();
    }
    hipError_t finish(hipStream_t s)
    {
        hipError_t e = moments ? mom.finish(s) : hipSuccess;
        if (e == hipSuccess) e = K.enqueue(s);
        return e;
    }
    int done() { return moments ? mom.done() : ST_OK; }
};

// run(chunk_pairs, reducer) is one compare_run over the caller's pairs.  chunk_pairs 0: one pass gives the moments and
// the keys.  Another chunk would change the order of the moments' float sums, so then the moments take a pass of their
// own at the path's default chunk and the keys a second one at chunk_pairs: out is always st_compare_*_host's.
template <typename Run>
static int compare_kendall(st_tree *tx, int64_t n, int64_t chunk_pairs, Run run, st_pair_moments *out, st_kendall_counts *out_counts)
{
    ST_DEVICE(tx->device);
    KendallState K;
    int rc = K.alloc(n);
    if (rc != ST_OK) return rc;
    if (chunk_pairs != 0) {
        MomentsReduce mom{nullptr, nullptr, 0, 0, out, nullptr};
        rc = run((int64_t)0, mom);
        if (rc != ST_OK) return rc;
    }
    KendallKeysReduce keys{MomentsReduce{nullptr, nullptr, 0, 0, out, nullptr}, K, chunk_pairs == 0};
    rc = run(chunk_pairs, keys);
    if (rc != ST_OK) return rc;
    K.done(out_counts);
    return ST_OK;
}

// st_kendall_arrays_host: the two columns are staged in the sort's second buffer (x in its first 4 n bytes, y in the
// last), their keys written to the first, then KendallState::enqueue as above.
static int kendall_arrays(int device, const float *x, const float *y, int64_t n, st_kendall_counts *out)
{
    ST_DEVICE(device);
    KendallState K;
    int rc = K.alloc(n);
    if (rc != ST_OK) return rc;
    DrainedStream s;
    float *d_x = reinterpret_cast<float *>(K.d_keys[1].get()), *d_y = d_x + n;
    hipError_t e = s.create();
    if (e == hipSuccess) e = K.start(s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_x, x, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_y, y, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_kendall_keys, dim3(K.grid()), dim3(kKendallThreads), 0, s, d_x, d_y, (long long)n, K.d_keys[0].get(), K.d_nan());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = K.enqueue(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("Kendall counts: ") + hipGetErrorString(e));
    K.done(out);
    return ST_OK;
}

// ---- the entry points: pair input x statistic (st_compare_{triangle,pairs}[_ranks|_kendall]_host) ----------------------
static int compare_trees_args(st_tree *tx, st_tree *ty)
{
    if (!tx || !ty) return fail(ST_ERR_ARG, "tree_x or tree_y is NULL");
    if (tx->device != ty->device)
        return fail(ST_ERR_ARG, "tree_x is on device " + std::to_string(tx->device) + ", tree_y on device " + std::to_string(ty->device) +
                                    ": both trees must live on the same device");
    return ST_OK;
}

static int chunk_pairs_arg(int64_t chunk_pairs)
{
    if (chunk_pairs >= 0 && chunk_pairs % ST_CLADE_TILE == 0) return ST_OK;
    return fail(ST_ERR_ARG, "chunk_pairs must be 0 or a positive multiple of " + std::to_string(ST_CLADE_TILE));
}

// the chunk, then the count (ranks and Kendall counts: at most 2^31 - 1 pairs)
static int rank_count_args(int64_t chunk_pairs, int64_t n, const char *what)
{
    const int rc = chunk_pairs_arg(chunk_pairs);
    if (rc != ST_OK || n <= kRankMaxPairs) return rc;
    return fail(ST_ERR_ARG, std::string(what) + " of " + std::to_string(n) + " pairs: at most " + std::to_string(kRankMaxPairs) + " (2^31 - 1)");
}

static int compare_empty(st_pair_moments *out, int64_t *out_hist, int32_t bins_x, int32_t bins_y)
{
    *out = moments_empty();
    if (out_hist) std::memset(out_hist, 0, (size_t)bins_x * (size_t)bins_y * 8);
    return ST_OK;
}

// A statistic holds its output pointers (and its chunk): out_args() checks them, count_args(n) what it asks of the pair
// count, empty() is the result of no pairs, go(tx, n, run) computes it -- run(chunk_pairs, reducer) is one compare_run
// over the caller's pairs.  A new statistic is one more such struct.
struct MomentsStat {
    const double *edges_x, *edges_y;
    int32_t bins_x, bins_y;
    st_pair_moments *out;
    int64_t *out_hist;

    int out_args() const
    {
        std::string err;
        const int rc = compare_hist_args(edges_x, bins_x, edges_y, bins_y, out_hist, kCmpMaxCells, err);
        if (rc != ST_OK) return fail(rc, err);
        return out ? ST_OK : fail(ST_ERR_ARG, "out is NULL");
    }
    int count_args(int64_t) const { return ST_OK; }
    int empty() const { return compare_empty(out, out_hist, bins_x, bins_y); }
    template <typename Run>
    int go(st_tree *, int64_t, Run run) const { MomentsReduce red{edges_x, edges_y, bins_x, bins_y, out, out_hist}; return run((int64_t)0, red); }
};

struct RanksStat {
    int64_t chunk_pairs;
    st_pair_moments *out;
    st_rank_sums *out_ranks;

    int out_args() const { return out && out_ranks ? ST_OK : fail(ST_ERR_ARG, "out or out_ranks is NULL"); }
    int count_args(int64_t n) const { return rank_count_args(chunk_pairs, n, "ranks"); }
    int empty() const { rank_finish(0, 0, 0, 0, 0, 0, 0, out_ranks); return compare_empty(out, nullptr, 0, 0); }
    template <typename Run>
    int go(st_tree *tx, int64_t n, Run run) const { return compare_ranks(tx, n, chunk_pairs, run, out, out_ranks); }
};

struct KendallStat {
    int64_t chunk_pairs;
    st_pair_moments *out;
    st_kendall_counts *out_counts;

    int out_args() const { return out && out_counts ? ST_OK : fail(ST_ERR_ARG, "out or out_counts is NULL"); }
    int count_args(int64_t n) const { return rank_count_args(chunk_pairs, n, "Kendall counts"); }
    int empty() const { kendall_finish(0, 0, 0, 0, 0, 0, out_counts); return compare_empty(out, nullptr, 0, 0); }
    template <typename Run>
    int go(st_tree *tx, int64_t n, Run run) const { return compare_kendall(tx, n, chunk_pairs, run, out, out_counts); }
};

// What every such entry point does, in the order in which its errors are reported: the statistic's outputs, the trees,
// the input's range, the chunk and the count, the NULL id arrays; then the empty result, or the ids (tree X's first) and
// the run.
template <typename In, typename Stat>
static int compare_entry(st_tree *tx, st_tree *ty, const In &in, Stat &&stat, int64_t *bad_id)
{
    int rc = stat.out_args();
    if (rc == ST_OK) rc = compare_trees_args(tx, ty);
    if (rc == ST_OK) rc = in.range_args();
    if (rc == ST_OK) rc = stat.count_args(in.count());
    if (rc == ST_OK) rc = in.null_args();
    if (rc != ST_OK) return rc;
    if (in.count() == 0) return stat.empty();
    rc = in.check_ids(tx, ty, bad_id);
    if (rc != ST_OK) return rc;
    return stat.go(tx, in.count(), [&](int64_t chunk, auto &red) { return in.run(tx, ty, chunk, red, bad_id); });
}
