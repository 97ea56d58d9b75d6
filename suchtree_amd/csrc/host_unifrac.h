// host_unifrac.h -- part of suchtree_hip.hip (included after host_dispersion.h).  The device side of st_unifrac_host and
// st_unifrac_depths (kernels_unifrac.h; the plan, the quantiser and the host restatement: unifrac_plan.cpp).  One work
// block: the heavy counter, the quantised depths, the range-minimum table (level 0 is h_q, one launch per further level),
// the positions and offsets, one heavy list and two chunks of int64 results.  Per chunk: the counter zeroed, the lane
// kernel, the wave kernel over what the lane kernel listed (skipped where no two sets reach the threshold), the results
// copied to one of two pinned buffers (ReadbackRing, host_compare.h) and moved to the caller's arrays while the device
// works on the next chunk.  st_unifrac_host first has the tree's distance and MRCA kernels write d and h, reads them back
// and quantises them on the host (at most 2 n values).
#pragma once

// the lane / wave threshold: ST_UNIFRAC_LANE_MAX, or SUCHTREE_AMD_UNIFRAC_LANE_MAX for a measurement (scripts/unifrac_bench.py
// sweeps it); no result depends on it
static int unifrac_lane_max()
{
    const char *e = std::getenv("SUCHTREE_AMD_UNIFRAC_LANE_MAX");
    if (e && *e) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end && *end == 0 && v >= 0 && v <= (1 << 22)) return (int)v;
    }
    return kUnifracLaneMax;
}

// The head of a UniFrac work block, which st_unifrac_* and st_unifrac_null_* lay out alike: the heavy counter in the block's
// first bytes, the quantised depths, the range-minimum table (level 0 is h_q), the positions and the set offsets; the caller
// lays out its own regions from `end`.  And the rule that decides whether a call has heavy pairs at all.
struct UnifracHead {
    size_t o_dq = 256, o_table = 0, o_pos = 0, o_sets = 0, end = 0;
    int lane_max = 0;
    bool heavy = false;      // (false: no task reaches the wave form, and its launch is left out)

    template <typename Plan>
    void lay_out(const Plan &P, int64_t n_pos, const int64_t *sets)
    {
        o_table = o_dq + align256((size_t)P.n * 8);
        o_pos = o_table + align256((size_t)P.levels * (size_t)P.m * 8);
        o_sets = o_pos + align256((size_t)n_pos * 4);
        end = o_sets + align256((size_t)(P.n_sets + 1) * 8);
        int64_t largest = 0;
        for (int64_t r = 0; r < P.n_sets; r++) largest = std::max(largest, sets[r + 1] - sets[r]);
        lane_max = unifrac_lane_max();
        heavy = 2 * largest > lane_max;
    }
    // the four uploads (host arrays that outlive the call's stream work) and the table's further levels on stream s
    template <typename Plan>
    int fill(char *d, const char *what, hipStream_t s, const Plan &P, const int64_t *d_q, const int64_t *h_q, const int32_t *set_pos, int64_t n_pos,
             const int64_t *sets) const
    {
        int64_t *const d_table = reinterpret_cast<int64_t *>(d + o_table);
        hipError_t e = hipMemcpyAsync(d + o_dq, d_q, (size_t)P.n * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && P.m > 0) e = hipMemcpyAsync(d_table, h_q, (size_t)P.m * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && n_pos > 0) e = hipMemcpyAsync(d + o_pos, set_pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_sets, sets, (size_t)(P.n_sets + 1) * 8, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
        for (int l = 1; l < P.levels; l++) {      // (2^l <= m: every level has an entry)
            const int64_t half = (int64_t)1 << (l - 1), count = P.m - 2 * half + 1;
            hipLaunchKernelGGL(k_unifrac_table, dim3((unsigned)((count + kUnifracThreads - 1) / kUnifracThreads)), dim3(kUnifracThreads), 0, s,
                               d_table + (int64_t)(l - 1) * P.m, d_table + (int64_t)l * P.m, (long long)half, (long long)count);
            e = hipGetLastError();
            if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
        }
        return ST_OK;
    }
};

using UnifracRing = ReadbackRing<int64_t, const UnifracChunk *>;

struct UnifracWork {      // declared before the stream's owner
    DevBuf<char> d;
    UnifracRing ring;
    UnifracHead H;
    size_t o_heavy = 0, o_out = 0, out_bytes = 0;

    // the status of alloc_work (host_compare.h): ST_ERR_NOMEM with the bytes asked for
    int alloc(const UnifracPlan &P, int64_t n_pos, const int64_t *sets, const char *what)
    {
        H.lay_out(P, n_pos, sets);
        o_heavy = H.end;
        o_out = o_heavy + align256((size_t)P.max_chunk * 4);
        out_bytes = align256((size_t)P.max_chunk * 8);
        return alloc_work(d, o_out + 2 * out_bytes, ring, (size_t)P.max_chunk, what);
    }
};

// every chunk of the plan on stream s over the quantised depths (host arrays that outlive the call's stream work).
// Returns ST_OK or ST_ERR_HIP; on return nothing of this call is pending on s unless a HIP call failed.
static int unifrac_chunks(UnifracWork &W, const char *what, hipStream_t s, const UnifracPlan &P, const int64_t *d_q, const int64_t *h_q,
                          const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t *out_pd, int64_t *out_union)
{
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    char *const d = W.d;
    const UnifracHead &H = W.H;
    if (const int rc = H.fill(d, what, s, P, d_q, h_q, set_pos, n_pos, sets); rc != ST_OK) return rc;
    hipError_t e = hipSuccess;
    int64_t *d_out[2] = {reinterpret_cast<int64_t *>(d + W.o_out), reinterpret_cast<int64_t *>(d + W.o_out + W.out_bytes)};
    auto deliver = [&](const int64_t *got, const UnifracChunk *c) {
        std::memcpy((c->kind == kUnifracPD ? out_pd : out_union) + c->out_at, got, (size_t)c->count * 8);
    };
    for (const UnifracChunk &c : P.chunks) {
        e = W.ring.acquire(deliver);      // (the results of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        int64_t *const out = d_out[W.ring.next];
        const UnifracArgs a{reinterpret_cast<const int64_t *>(d + H.o_dq), reinterpret_cast<const int64_t *>(d + H.o_table),
                            reinterpret_cast<const int *>(d + H.o_pos), reinterpret_cast<const int64_t *>(d + H.o_sets), out,
                            reinterpret_cast<unsigned *>(d + W.o_heavy), reinterpret_cast<unsigned *>(d), (long long)P.m, (long long)c.begin,
                            (unsigned)c.count, c.kind, H.lane_max};
        if (H.heavy) e = hipMemsetAsync(d, 0, 16, s);      // (stream order: the wave kernel of the chunk before has read it)
        if (e != hipSuccess) return hip_fail(" launch: ", e);
        hipLaunchKernelGGL(k_unifrac_lane, dim3((unsigned)((c.count + kUnifracThreads - 1) / kUnifracThreads)), dim3(kUnifracThreads), 0, s, a);
        e = hipGetLastError();
        if (e == hipSuccess && H.heavy) {
            hipLaunchKernelGGL(k_unifrac_wave, dim3(kUnifracWaveBlocks), dim3(kUnifracThreads), 0, s, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = W.ring.post(out, (size_t)c.count, &c, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    e = W.ring.drain(deliver, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}

static int unifrac_depths_device(int device, const UnifracPlan &P, const int64_t *d_q, const int64_t *h_q, const int32_t *set_pos, int64_t n_pos,
                                 const int64_t *sets, int64_t *out_pd, int64_t *out_union)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    UnifracWork W;
    DrainedStream s;
    const hipError_t e = s.create();
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("unifrac depths setup: ") + hipGetErrorString(e));
    if (const int rc = W.alloc(P, n_pos, sets, "unifrac depths"); rc != ST_OK) return rc;
    return unifrac_chunks(W, "unifrac depths", s, P, d_q, h_q, set_pos, n_pos, sets, out_pd, out_union);
}

struct UnifracDepths {      // read-back targets: declared before the stream's owner
    std::vector<float> d, h;            // d[k] = dist(root, u[k]); h[k] = dist(root, mrca(u[k], u[k + 1]))
    std::vector<int64_t> d_q, h_q;      // quantised by unifrac_quantise with the caller's shift ...
    int32_t shift = 0;                  // ... the shift used
};

// The depths of the n ids of `univ` below `root` in the tree of the session `ses`: its depth block and stream opened, the
// tree's distance and MRCA kernels, the read-back, the session closed (the stream drained), the values quantised on the host.
static int unifrac_tree_depths(TwoTreeSession &ses, st_tree *t, int64_t root, const int64_t *univ, int32_t n_univ, int32_t shift, UnifracDepths &Z,
                               int64_t *bad_id)
{
    const size_t n = (size_t)n_univ, m = n - 1;
    Z.d.resize(n);
    Z.h.resize(m);
    // the depth block: root | universe | d | MRCA ids of adjacent leaves, as int32 and as int64 | h
    const size_t o_univ = 256, o_d = o_univ + align256(n * 8), o_m32 = o_d + align256(n * 4), o_m64 = o_m32 + align256(m * 4);
    const size_t o_h = o_m64 + align256(m * 8), total = o_h + align256(m * 4);
    int rc = ses.open_or_nomem(total, "a depth block");
    if (rc != ST_OK) return rc;
    char *const d = ses.d;
    const hipStream_t s = ses.s;
    long long *d_root = reinterpret_cast<long long *>(d), *d_univ = reinterpret_cast<long long *>(d + o_univ);
    long long *d_m64 = reinterpret_cast<long long *>(d + o_m64);
    int *d_m32 = reinterpret_cast<int *>(d + o_m32);
    float *d_d = reinterpret_cast<float *>(d + o_d), *d_h = reinterpret_cast<float *>(d + o_h);
    const long long root_id = root;
    hipError_t e = hipMemcpyAsync(d_root, &root_id, 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_univ, univ, n * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    rc = ses.arm();
    if (rc != ST_OK) return rc;
    // d[k] = dist(root, u[k]), the arguments in that order: a 1 x n grid
    rc = enqueue_grid_dist(t, d_root, d_univ, n, n, d_d, s);
    if (rc != ST_OK) return rc;
    if (m > 0) {      // h[k] = dist(root, mrca(u[k], u[k + 1])): the pairs are the universe read with stride one
        rc = enqueue_src(t, SrcStrided{d_univ, 1, 1}, (int64_t)m, DistSink{nullptr, nullptr}, MrcaSink{d_m32, nullptr}, t->d_fault_host, s);
        if (rc != ST_OK) return rc;
        hipLaunchKernelGGL(k_unifrac_widen, dim3((unsigned)((m + kUnifracThreads - 1) / kUnifracThreads)), dim3(kUnifracThreads), 0, s, d_m32, d_m64,
                           (long long)m);
        e = hipGetLastError();
        if (e != hipSuccess) return ses.hip_fail(" launch: ", e);
        rc = enqueue_grid_dist(t, d_root, d_m64, m, m, d_h, s);
        if (rc != ST_OK) return rc;
        e = hipMemcpyAsync(Z.h.data(), d_h, m * 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(Z.d.data(), d_d, n * 4, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    rc = ses.close(bad_id);      // (drains the stream)
    if (rc != ST_OK) return rc;
    Z.d_q.resize(n);
    Z.h_q.resize(m);
    std::string err;
    rc = unifrac_quantise(Z.d.data(), Z.h.data(), n_univ, shift, Z.d_q.data(), Z.h_q.data(), &Z.shift, err);
    return rc == ST_OK ? ST_OK : fail(rc, err);
}

static int unifrac_tree_run(st_tree *t, int64_t root, const int64_t *univ, const UnifracPlan &P, const int32_t *set_pos, int64_t n_pos,
                            const int64_t *sets, int32_t shift, int64_t *out_pd, int64_t *out_union, int32_t *out_shift, float *out_d, float *out_h,
                            int64_t *bad_id)
{
    ST_DEVICE(t->device);
    UnifracDepths Z;
    UnifracWork W;
    TwoTreeSession ses(t, t, "unifrac");
    int rc = P.chunks.empty() ? ST_OK : W.alloc(P, n_pos, sets, "unifrac");
    if (rc == ST_OK) rc = unifrac_tree_depths(ses, t, root, univ, P.n, shift, Z, bad_id);
    if (rc != ST_OK) return rc;
    if (out_shift) *out_shift = Z.shift;
    if (out_d) std::copy(Z.d.begin(), Z.d.end(), out_d);
    if (out_h) std::copy(Z.h.begin(), Z.h.end(), out_h);
    if (P.chunks.empty()) return ST_OK;
    return unifrac_chunks(W, "unifrac", ses.s, P, Z.d_q.data(), Z.h_q.data(), set_pos, n_pos, sets, out_pd, out_union);
}
