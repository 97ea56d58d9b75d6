// host_dispersion.h -- part of suchtree_hip.hip (included after host_hommola.h).  The device side of
// st_partner_dispersion_host and st_dispersion_matrix (kernels_dispersion.h; the plan, the host restatement and the
// scatter: dispersion_plan.cpp).  The float32 matrix D is the caller's, uploaded, or written once by the unchanged
// distance kernels over a SrcGrid.  One work block beside it: the positions, the set table, one block of sigma rows and
// two chunks of records.  Per block of permutations: its sorts (k_dispersion_sigma); per chunk of whole tasks: one launch
// per size class it meets (k_dispersion_tasks_*), its records copied to one of two pinned buffers (ReadbackRing,
// host_compare.h) and scattered to the caller's rows while the device works on the next chunk.
#pragma once

using DispersionRing = ReadbackRing<st_dispersion_record, const DispersionChunk *>;

static hipError_t dispersion_launch_sigma(const DispersionSigmaArgs &a, int64_t n_perms, hipStream_t s)
{
    const int cls = perm_sort_class(a.n);
    if (cls == kPermSortLarge) {
        hipLaunchKernelGGL(k_dispersion_sigma<kPermLargeThreads>, dim3((unsigned)n_perms), dim3(kPermLargeThreads), perm_lds_bytes(a.n), s, a);
    } else {
        hipLaunchKernelGGL(k_dispersion_sigma<kPermSmallThreads>, dim3((unsigned)n_perms), dim3(kPermSmallThreads),
                           cls == kPermSortWave ? 0 : perm_lds_bytes(a.n), s, a);
    }
    return hipGetLastError();
}

// the launches of tasks [c.task_begin, c.task_begin + c.n_tasks): one per size class whose range of tasks meets the chunk
static hipError_t dispersion_launch_tasks(const DispersionPlan &P, const DispersionChunk &c, DispersionTaskArgs a, hipStream_t s)
{
    st_dispersion_record *const rec = a.out;      // the chunk's records: entry t - c.task_begin

    const int64_t lo = c.task_begin, hi = c.task_begin + c.n_tasks, per = kDispersionThreads / 64;
    for (int k = 0; k < kDispersionClasses; k++) {
        const int64_t b = std::max(lo, P.class_begin[k] * c.n_perms), e = std::min(hi, P.class_begin[k + 1] * c.n_perms);
        if (e <= b) continue;
        a.set0 = b / c.n_perms;
        a.perm0 = (unsigned)(b - a.set0 * c.n_perms);
        a.n = e - b;
        a.out = rec + (b - lo);
        a.lanes = 2 << k;
        if (a.lanes <= kDispersionPackedMax) {
            const int64_t waves = (a.n + 64 / a.lanes - 1) / (64 / a.lanes);
            hipLaunchKernelGGL(k_dispersion_tasks_packed, dim3((unsigned)((waves + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else if (k == 5) {
            hipLaunchKernelGGL(k_dispersion_tasks_wave, dim3((unsigned)((a.n + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else {
            const size_t lds = (((size_t)P.max_count + 7) & ~(size_t)7) * 2;
            hipLaunchKernelGGL(k_dispersion_tasks_group, dim3((unsigned)a.n), dim3(kDispersionThreads), lds, s, a);
        }
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    return hipSuccess;
}

// Every chunk of a plan of (table entry, permutation) tasks -- DispersionPlan over its sets, SetpairPlan over its
// directions -- on stream s, with the caller's work block and ring (declared before the
// stream's owner); `what` names the call in messages.  `table` is uploaded beside the positions; launch(chunk, sigma,
// set_pos, table, records, stream) enqueues a chunk's kernels, scatter(records, chunk) puts its records into the
// caller's `out` of n_out records.  Returns ST_OK, ST_ERR_NOMEM or ST_ERR_HIP; on return nothing of this call is pending
// on s unless a HIP call failed.
template <typename Plan, typename Item, typename Launch, typename Scatter>
static int dispersion_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const Plan &P, const std::vector<Item> &table,
                             const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out, int64_t n_out,
                             Launch launch, Scatter scatter_to)
{
    const size_t n = (size_t)P.n_univ, live = table.size();
    const size_t o_sets = align256((size_t)n_pos * 4), o_sigma = o_sets + align256(live * sizeof(Item));
    const size_t rec_bytes = align256((size_t)P.max_chunk_tasks * sizeof(st_dispersion_record));
    const size_t o_rec = o_sigma + align256((size_t)P.perm_block * n * 2), total = o_rec + 2 * rec_bytes;
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    if (const int rc = alloc_work(d_work, total, ring, (size_t)P.max_chunk_tasks, what); rc != ST_OK) return rc;
    std::fill_n(out, n_out, st_dispersion_record{0.0, 0.0});      // (every allocation has succeeded: from here on out is written)
    char *const d = d_work;
    st_dispersion_record *d_rec[2] = {reinterpret_cast<st_dispersion_record *>(d + o_rec), reinterpret_cast<st_dispersion_record *>(d + o_rec + rec_bytes)};
    hipError_t e = hipMemcpyAsync(d, set_pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_sets, table.data(), live * sizeof(Item), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    auto scatter = [&](const st_dispersion_record *records, const DispersionChunk *c) { scatter_to(records, *c); };
    int64_t sigma_p = -1;      // the block whose rows the device holds
    for (const DispersionChunk &c : P.chunks) {
        e = ring.acquire(scatter);      // (the records of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        st_dispersion_record *const d_out = d_rec[ring.next];
        if (c.p_begin != sigma_p) {      // (stream order: the tasks of the block before have read their rows)
            e = dispersion_launch_sigma(DispersionSigmaArgs{reinterpret_cast<unsigned short *>(d + o_sigma), (long long)c.p_begin, (unsigned long long)seed,
                                                            (int)stream, (int)n},
                                        c.n_perms, s);
            if (e != hipSuccess) return hip_fail(" launch: ", e);
            sigma_p = c.p_begin;
        }
        e = launch(c, reinterpret_cast<const unsigned short *>(d + o_sigma), reinterpret_cast<const int *>(d), reinterpret_cast<const Item *>(d + o_sets),
                   d_out, s);
        if (e == hipSuccess) e = ring.post(d_out, (size_t)c.n_tasks, &c, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    e = ring.drain(scatter, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}

// the dispersion call's chunks: the live sets as the table, dispersion_launch_tasks, dispersion_scatter
static int dispersion_run_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const float *d_D, const DispersionPlan &P,
                                 const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out)
{
    return dispersion_chunks(
        d_work, ring, what, s, P, P.sets, set_pos, n_pos, seed, stream, out, P.n_sets * P.rows,
        [&](const DispersionChunk &c, const unsigned short *sigma, const int *pos, const DispersionSetDev *sets, st_dispersion_record *d_out, hipStream_t st) {
            return dispersion_launch_tasks(P, c, DispersionTaskArgs{d_D, sigma, pos, sets, d_out, 0, 0, 0, (unsigned)c.n_perms, P.n_univ, 0}, st);
        },
        [&](const st_dispersion_record *records, const DispersionChunk &c) { dispersion_scatter(P, c, records, out); });
}

// D[a][b] = dist(u[a], u[b]) as float32, the arguments in that order (not symmetric in the last bit), over the n ids of
// `univ`: the session's block and stream opened, the fault words armed, the distance kernels enqueued
static int dispersion_build_matrix(TwoTreeSession &ses, st_tree *t, const int64_t *univ, size_t n, const float *&d_D)
{
    const size_t o_univ = align256(n * n * 4), total = o_univ + align256(n * 8);
    int rc = ses.open_or_nomem(total, "a distance matrix");
    if (rc != ST_OK) return rc;
    char *const d = ses.d;
    long long *d_univ = reinterpret_cast<long long *>(d + o_univ);
    const hipError_t e = hipMemcpyAsync(d_univ, univ, n * 8, hipMemcpyHostToDevice, ses.s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    rc = ses.arm();
    if (rc != ST_OK) return rc;
    d_D = reinterpret_cast<float *>(d);
    return enqueue_grid_dist(t, d_univ, d_univ, n, n * n, reinterpret_cast<float *>(d), ses.s);
}

static int partner_dispersion_run(st_tree *t, const int64_t *univ, const DispersionPlan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed,
                                  int32_t stream, st_dispersion_record *out, int64_t *bad_id)
{
    ST_DEVICE(t->device);
    DevBuf<char> d_work;
    DispersionRing ring;
    TwoTreeSession ses(t, t, "partner dispersion");
    const float *d_D = nullptr;
    int rc = dispersion_build_matrix(ses, t, univ, (size_t)P.n_univ, d_D);
    if (rc != ST_OK) return rc;
    rc = dispersion_run_chunks(d_work, ring, "partner dispersion", ses.s, d_D, P, set_pos, n_pos, seed, stream, out);
    if (rc != ST_OK) return rc;
    return ses.close(bad_id);
}

// the caller's matrix D (n x n float32) on `device`, uploaded on the stream s (created here)
static int dispersion_upload_matrix(const char *what, const float *D, size_t n, DevBuf<float> &d_D, DrainedStream &s)
{
    hipError_t e = s.create();
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    e = d_D.alloc(n * n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ST_ERR_NOMEM, std::string(what) + ": a matrix of " + std::to_string(n * n * 4) + " bytes: " + hipGetErrorString(e));
    }
    e = hipMemcpyAsync(d_D, D, n * n * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " upload: " + hipGetErrorString(e));
    return ST_OK;
}

static int dispersion_matrix_device(int device, const float *D, const DispersionPlan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed,
                                    int32_t stream, st_dispersion_record *out)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DispersionRing ring;
    DevBuf<float> d_D;
    DrainedStream s;
    if (const int rc = dispersion_upload_matrix("dispersion matrix", D, (size_t)P.n_univ, d_D, s); rc != ST_OK) return rc;
    return dispersion_run_chunks(d_work, ring, "dispersion matrix", s, d_D, P, set_pos, n_pos, seed, stream, out);
}
