// host_misc.h -- part of suchtree_hip.hip (included after host_path.h).  The drivers of kernels_misc.h, each behind its
// export's checks: the 24-bit id unpack (st_unpack_mrca24_device), k nearest (st_knn_host), the dense graph matrices
// (st_graph_matrices_host).
#pragma once

static int unpack_mrca24_run(int device, const uint8_t *d_packed, int64_t n, int32_t *d_out_mrca, void *stream)
{
    ST_DEVICE(device);
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_unpack24, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_packed, (long long)n, d_out_mrca);
    ST_HIP(hipGetLastError());
    return ST_OK;
}

// n_queries > 0 rows over n_cands > 0 candidates: blocks of rows through the handle's distance kernels over SrcGrid, then the
// selection of each row's k nearest
static int knn_host_run(st_tree *t, const int64_t *queries, int64_t n_queries, const int64_t *cands, int64_t n_cands, int k, int skip_self,
                        int64_t *out_index, double *out_dist, int64_t *bad_id)
{
    ST_DEVICE(t->device);
    std::lock_guard<std::mutex> lock(t->dp->m);
    // rows per launch: the distance block (float32, device only) stays under 256 MiB
    const int64_t rows_per_block = std::max<int64_t>(1, std::min<int64_t>(n_queries, ((int64_t)1 << 26) / n_cands));
    DevBuf<long long> d_q, d_c, d_oi;
    DevBuf<float> d_tmp;
    DevBuf<double> d_od;
    DrainedStream stream;      // (every way out drains it before the buffers go)
    hipError_t e = stream.create();
    if (e == hipSuccess) e = d_q.alloc((size_t)n_queries);
    if (e == hipSuccess) e = d_c.alloc((size_t)n_cands);
    if (e == hipSuccess) e = d_tmp.alloc((size_t)rows_per_block * (size_t)n_cands);
    if (e == hipSuccess) e = d_oi.alloc((size_t)n_queries * k);
    if (e == hipSuccess) e = d_od.alloc((size_t)n_queries * k);
    if (e == hipSuccess) e = hipMemcpyAsync(d_q, queries, (size_t)n_queries * 8, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_c, cands, (size_t)n_cands * 8, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("knn setup: ") + hipGetErrorString(e));
    if (begin_host_faults(t, stream) != ST_OK) return ST_ERR_HIP;
    for (int64_t r0 = 0; r0 < n_queries; r0 += rows_per_block) {
        const int64_t rows = std::min(rows_per_block, n_queries - r0);
        const SrcGrid src{d_q + r0, d_c, (long long)n_cands, 0, 0};
        const int rc = enqueue_src(t, src, rows * n_cands, DistSink{nullptr, d_tmp}, MrcaSink{nullptr, nullptr}, t->d_fault_host, stream);
        if (rc != ST_OK) return rc;
        hipLaunchKernelGGL(k_knn_select, dim3((unsigned)rows), dim3(256), 0, stream, d_tmp, (long long)n_cands,
                           d_q + r0, d_c, skip_self, k, d_oi + r0 * k, d_od + r0 * k);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("knn launch: ") + hipGetErrorString(e));
    }
    e = hipMemcpyAsync(out_index, d_oi, (size_t)n_queries * k * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_dist, d_od, (size_t)n_queries * k * 8, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("knn D2H: ") + hipGetErrorString(e));
    Fault f = kFaultInit;
    const int rc = end_host_faults(t, stream, f);
    if (rc != ST_OK) return rc;
    return report_fault(t->n_nodes, f, bad_id);
}

// adjacency and / or Laplacian of n nodes from a checked edge list, on `device`
static int graph_matrices_run(int device, int64_t n, int64_t n_edges, const int32_t *u, const int32_t *v, const double *w, double *out_adjacency,
                              double *out_laplacian)
{
    ST_DEVICE(device);
    // one workspace: A, L (only if asked for), column sums, edge list.  The dense matrices
    // must fit the GPU's free memory with room to spare; beyond that the caller should not
    // be building a dense Laplacian at all (the reference's numpy version would need the same
    // bytes of host memory).
    const size_t mat = (size_t)n * (size_t)n * 8;
    const size_t edges_b = (size_t)std::max<int64_t>(n_edges, 1);
    const size_t need = mat * (out_laplacian ? 2 : 1) + (size_t)n * 8 + edges_b * 16 + 4096;
    size_t free_b = 0, total_b = 0;
    ST_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b / 10 * 9)
        return fail(ST_ERR_NOMEM, "dense " + std::to_string(n) + " x " + std::to_string(n) + " graph matrices need " +
                                      std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB free");
    // one grow-only workspace per device, kept between calls (a 422 x 422 Laplacian is all
    // allocation time otherwise); calls on one device take turns
    struct Workspace { std::mutex m; DevBuf<char> p; size_t cap = 0; };      // (never deleted: no HIP call from a static destructor)
    static std::mutex ws_map_mutex;
    static std::map<int, Workspace *> ws_map;
    Workspace *W;
    {
        std::lock_guard<std::mutex> g(ws_map_mutex);
        Workspace *&slot = ws_map[device];
        if (!slot) slot = new Workspace();
        W = slot;
    }
    std::lock_guard<std::mutex> ws_lock(W->m);
    if (W->cap < need) {
        W->cap = 0;
        ST_HIP(W->p.alloc(need));
        W->cap = need;
    }
    char *ws = W->p;
    double *d_A = reinterpret_cast<double *>(ws);
    double *d_L = out_laplacian ? d_A + (size_t)n * n : nullptr;
    double *d_deg = reinterpret_cast<double *>(ws + mat * (out_laplacian ? 2 : 1));
    double *d_w = d_deg + n;
    int *d_u = reinterpret_cast<int *>(d_w + edges_b), *d_v = d_u + edges_b;
    hipError_t e = hipMemsetAsync(d_A, 0, mat, nullptr);
    if (e == hipSuccess && n_edges) e = hipMemcpyAsync(d_u, u, (size_t)n_edges * 4, hipMemcpyHostToDevice, nullptr);
    if (e == hipSuccess && n_edges) e = hipMemcpyAsync(d_v, v, (size_t)n_edges * 4, hipMemcpyHostToDevice, nullptr);
    if (e == hipSuccess && n_edges) e = hipMemcpyAsync(d_w, w, (size_t)n_edges * 8, hipMemcpyHostToDevice, nullptr);
    if (e == hipSuccess) {
        if (n_edges)
            hipLaunchKernelGGL(k_graph_scatter, dim3((unsigned)std::min<int64_t>((n_edges + 255) / 256, 4096)),
                               dim3(256), 0, nullptr, d_A, (long long)n, (long long)n_edges, d_u, d_v, d_w);
        if (out_laplacian) {
            // one lane per column, rows in increasing order (numpy's sum(axis=0) order); waves of
            // 64 consecutive columns read each row coalesced, one wave per workgroup so that a
            // few hundred columns already spread over the chip
            hipLaunchKernelGGL(k_graph_degree, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, d_A, (long long)n, d_deg);
            hipLaunchKernelGGL(k_graph_laplacian, dim3((unsigned)std::min<int64_t>((n * n + 255) / 256, 65536)),
                               dim3(256), 0, nullptr, d_A, d_deg, (long long)n, d_L);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess && out_adjacency) e = hipMemcpy(out_adjacency, d_A, mat, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_laplacian) e = hipMemcpy(out_laplacian, d_L, mat, hipMemcpyDeviceToHost);
    if (W->cap > ((size_t)256 << 20)) {     // do not sit on a multi-GB workspace
        W->p.reset();
        W->cap = 0;
    }
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("graph matrices: ") + hipGetErrorString(e));
    return ST_OK;
}
