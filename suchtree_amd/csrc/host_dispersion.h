// host_dispersion.h -- part of suchtree_hip.hip (included after host_hommola.h).  The device side of the two passes that
// write records: st_partner_dispersion_host and st_dispersion_matrix (kernels_dispersion.h; the plan and the host
// restatement: dispersion_plan.cpp), st_beta_dispersion_host and st_beta_dispersion_matrix (kernels_setpair.h;
// setpair_plan.cpp).  They differ in the table beside the positions and in the three task kernels; the loop over blocks of
// permutations and their chunks (perm_block_chunks) also serves host_unifrac_null.h.  The float32 matrix D is the caller's, uploaded, or written once by the unchanged
// distance kernels over a SrcGrid.  One work block beside it: the positions, the set table, one block of sigma rows and
// two chunks of records.  Per block of permutations: its sorts (k_dispersion_sigma); per chunk of whole tasks: one launch
// per size class it meets (k_dispersion_tasks_*, k_setpair_tasks_*), its records copied to one of two pinned buffers (ReadbackRing,
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

// the launches of tasks [c.task_begin, c.task_begin + c.n_tasks) of a plan's size classes: one per class whose range of tasks
// meets the chunk.  `first` is the argument that takes a launch's first item; group_lds(lds) gives the workgroup form's LDS
// bytes, with whatever that kernel needs before it is launched with them.
template <typename Args, typename GroupLds>
static hipError_t dispersion_launch_tasks(const int64_t *class_begin, const DispersionChunk &c, Args a, long long Args::*first, void (*packed)(Args),
                                          void (*wave)(Args), void (*group)(Args), GroupLds group_lds, hipStream_t s)
{
    st_dispersion_record *const rec = a.out;      // the chunk's records: entry t - c.task_begin

    const int64_t lo = c.task_begin, hi = c.task_begin + c.n_tasks, per = kDispersionThreads / 64;
    for (int k = 0; k < kDispersionClasses; k++) {
        const int64_t b = std::max(lo, class_begin[k] * c.n_perms), e = std::min(hi, class_begin[k + 1] * c.n_perms);
        if (e <= b) continue;
        a.*first = b / c.n_perms;
        a.perm0 = (unsigned)(b - a.*first * c.n_perms);
        a.n = e - b;
        a.out = rec + (b - lo);
        a.lanes = 2 << k;
        if (a.lanes <= kDispersionPackedMax) {
            const int64_t waves = (a.n + 64 / a.lanes - 1) / (64 / a.lanes);
            hipLaunchKernelGGL(packed, dim3((unsigned)((waves + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else if (k == 5) {
            hipLaunchKernelGGL(wave, dim3((unsigned)((a.n + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else {
            size_t lds = 0;
            const hipError_t e1 = group_lds(lds);
            if (e1 != hipSuccess) return e1;
            hipLaunchKernelGGL(group, dim3((unsigned)a.n), dim3(kDispersionThreads), lds, s, a);
        }
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    return hipSuccess;
}

// Every chunk of a plan cut by dispersion_cut (DispersionPlan, SetpairPlan, UnifracNullPlan) on stream s: the one loop
// over blocks of permutations and their chunks.  The caller owns the work block and hands over what the loop touches of
// it: the block's sigma rows (d_sigma, sorted here when the block changes) and the device twins of the ring's two slots
// (d_out).  launch(chunk, results, stream) enqueues a chunk's kernels, scatter_to(results, chunk) puts its results where
// the caller wants them; `what` names the call in messages.  Returns ST_OK or ST_ERR_HIP; on return nothing of this call
// is pending on s unless a HIP call failed.
// The block's rows come from produce(chunk, stream), enqueued when the block changes: the sigma sorts (perm_block_chunks
// below), or the chains of the swap null (host_swap.h).
template <typename T, typename Produce, typename Launch, typename Scatter>
static int perm_block_chunks_of(ReadbackRing<T, const DispersionChunk *> &ring, const char *what, hipStream_t s, const std::vector<DispersionChunk> &chunks,
                                T *const (&d_out)[2], Produce produce, Launch launch, Scatter scatter_to)
{
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    auto scatter = [&](const T *results, const DispersionChunk *c) { scatter_to(results, *c); };
    int64_t sigma_p = -1;      // the block whose rows the device holds
    for (const DispersionChunk &c : chunks) {
        hipError_t e = ring.acquire(scatter);      // (the results of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        T *const out = d_out[ring.next];
        if (c.p_begin != sigma_p) {      // (stream order: the tasks of the block before have read their rows)
            e = produce(c, s);
            if (e != hipSuccess) return hip_fail(" launch: ", e);
            sigma_p = c.p_begin;
        }
        e = launch(c, out, s);
        if (e == hipSuccess) e = ring.post(out, (size_t)c.n_tasks, &c, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    const hipError_t e = ring.drain(scatter, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}

template <typename T, typename Launch, typename Scatter>
static int perm_block_chunks(ReadbackRing<T, const DispersionChunk *> &ring, const char *what, hipStream_t s, const std::vector<DispersionChunk> &chunks,
                             unsigned short *d_sigma, T *const (&d_out)[2], int32_t n_univ, uint64_t seed, int32_t stream, Launch launch,
                             Scatter scatter_to)
{
    return perm_block_chunks_of(
        ring, what, s, chunks, d_out,
        [&](const DispersionChunk &c, hipStream_t st) {
            return dispersion_launch_sigma(DispersionSigmaArgs{d_sigma, (long long)c.p_begin, (unsigned long long)seed, (int)stream, (int)n_univ}, c.n_perms, st);
        },
        launch, scatter_to);
}

// Every chunk of a matrix plan (MatrixPlan, dispersion_plan.h: host_mantel.h, host_group.h, host_class.h, host_parafit.h)
// on stream s: the loop over blocks of permutations and their chunks of the calls that fold a block on the device and
// read nothing back per chunk (which is why it is not perm_block_chunks_of: no ring).  produce(chunk, stream) enqueues a
// new block's rows, launch(chunk, stream) a chunk's tasks, fold(chunk) whatever completes the block of its last chunk.
// Stream order carries the loop: a block's fold is enqueued after its last chunk and before the next block's rows, so it
// reads what the block's tasks left, and the rows that those tasks read are overwritten only behind them.  A fold that
// hands a block to the host (ParaFit's link records) synchronises before it returns.  Returns ST_OK, or ST_ERR_HIP with
// `what` and " launch: "; the read-back is the caller's.
template <typename Produce, typename Launch, typename Fold>
static int matrix_block_chunks(const char *what, hipStream_t s, const std::vector<DispersionChunk> &chunks, Produce produce, Launch launch, Fold fold)
{
    hipError_t e = hipSuccess;
    const DispersionChunk *prev = nullptr;
    for (const DispersionChunk &c : chunks) {
        if (!prev || c.p_begin != prev->p_begin) {
            if (prev) e = fold(*prev);
            if (e == hipSuccess) e = produce(c, s);
        }
        if (e == hipSuccess) e = launch(c, s);
        if (e != hipSuccess) break;
        prev = &c;
    }
    if (e == hipSuccess && prev) e = fold(*prev);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return ST_OK;
}

// the stream and the work block of `total` bytes of such a call (the caller declares d_work before s): ST_OK, ST_ERR_HIP
// or ST_ERR_NOMEM
static int open_work_block(const char *what, DrainedStream &s, DevBuf<char> &d_work, size_t total)
{
    hipError_t e = s.create();
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    e = d_work.alloc(total);
    if (e == hipSuccess) return ST_OK;
    (void)hipGetLastError();
    return fail(ST_ERR_NOMEM, std::string(what) + ": a work block of " + std::to_string(total) + " bytes: " + hipGetErrorString(e));
}

// the permutations per task of a sliced plan: `dflt`, or the environment variable `name` = 1 .. max (read at every call; a
// measurement's: no result depends on it; anything else falls back to dflt)
static int32_t perm_slice_env(const char *name, int32_t dflt, int32_t max)
{
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    char *end = nullptr;
    const long s = std::strtol(v, &end, 10);
    return (*end == 0 && s >= 1 && s <= max) ? (int32_t)s : dflt;
}

// A plan of records -- DispersionPlan over its sets, SetpairPlan over its directions -- on stream s, with the caller's work
// block and ring (declared before the stream's owner): the positions, `table` beside them, one block of sigma rows and two
// chunks of records, then perm_block_chunks.  launch(chunk, sigma, set_pos, table, records, stream) enqueues a chunk's
// kernels; its records are scattered into the caller's `out` of n_out records (dispersion_scatter).  Returns ST_OK,
// ST_ERR_NOMEM or ST_ERR_HIP.
template <typename Plan, typename Item, typename Launch>
static int dispersion_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const Plan &P, const std::vector<Item> &table,
                             const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out, int64_t n_out,
                             Launch launch)
{
    const size_t n = (size_t)P.n_univ, live = table.size();
    const size_t o_sets = align256((size_t)n_pos * 4), o_sigma = o_sets + align256(live * sizeof(Item));
    const size_t rec_bytes = align256((size_t)P.max_chunk_tasks * sizeof(st_dispersion_record));
    const size_t o_rec = o_sigma + align256((size_t)P.perm_block * n * 2), total = o_rec + 2 * rec_bytes;
    if (const int rc = alloc_work(d_work, total, ring, (size_t)P.max_chunk_tasks, what); rc != ST_OK) return rc;
    std::fill_n(out, n_out, st_dispersion_record{0.0, 0.0});      // (every allocation has succeeded: from here on out is written)
    char *const d = d_work;
    st_dispersion_record *const d_rec[2] = {reinterpret_cast<st_dispersion_record *>(d + o_rec),
                                            reinterpret_cast<st_dispersion_record *>(d + o_rec + rec_bytes)};
    unsigned short *const d_sigma = reinterpret_cast<unsigned short *>(d + o_sigma);
    hipError_t e = hipMemcpyAsync(d, set_pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_sets, table.data(), live * sizeof(Item), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    return perm_block_chunks(
        ring, what, s, P.chunks, d_sigma, d_rec, P.n_univ, seed, stream,
        [&](const DispersionChunk &c, st_dispersion_record *d_out, hipStream_t st) {
            return launch(c, d_sigma, reinterpret_cast<const int *>(d), reinterpret_cast<const Item *>(d + o_sets), d_out, st);
        },
        [&](const st_dispersion_record *records, const DispersionChunk &c) { dispersion_scatter(P, c, records, out); });
}

// the dispersion call's chunks: the live sets as the table, the three k_dispersion_tasks_* forms
static int record_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const float *d_D, const DispersionPlan &P,
                         const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out)
{
    return dispersion_chunks(
        d_work, ring, what, s, P, P.sets, set_pos, n_pos, seed, stream, out, P.n_sets * P.rows,
        [&](const DispersionChunk &c, const unsigned short *sigma, const int *pos, const DispersionSetDev *sets, st_dispersion_record *d_out, hipStream_t st) {
            return dispersion_launch_tasks(
                P.class_begin, c, DispersionTaskArgs{d_D, sigma, pos, sets, d_out, 0, 0, 0, (unsigned)c.n_perms, P.n_univ, 0}, &DispersionTaskArgs::set0,
                k_dispersion_tasks_packed, k_dispersion_tasks_wave, k_dispersion_tasks_group,
                [&](size_t &lds) {
                    lds = (((size_t)P.max_count + 7) & ~(size_t)7) * 2;
                    return hipSuccess;
                },
                st);
        });
}

// the between-set call's chunks (kernels_setpair.h): the live directions as the table, the three k_setpair_tasks_* forms
static int record_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const float *d_D, const SetpairPlan &P,
                         const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out)
{
    return dispersion_chunks(
        d_work, ring, what, s, P, P.tasks, set_pos, n_pos, seed, stream, out, 2 * P.count * P.rows,
        [&](const DispersionChunk &c, const unsigned short *sigma, const int *pos, const SetpairTaskDev *tasks, st_dispersion_record *d_out, hipStream_t st) {
            return dispersion_launch_tasks(
                P.class_begin, c, SetpairTaskArgs{d_D, sigma, pos, tasks, d_out, 0, 0, 0, (unsigned)c.n_perms, P.n_univ, 0, P.exclude},
                &SetpairTaskArgs::task0, k_setpair_tasks_packed, k_setpair_tasks_wave, k_setpair_tasks_group,
                [&](size_t &lds) {
                    lds = setpair_lds_bytes(P.max_walk, P.exclude != 0);      // (up to 64 KiB: above 32 KiB they are asked for)
                    return perm_lds_opt_in(k_setpair_tasks_group, lds);
                },
                st);
        });
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

// a plan of records (record_chunks) over the matrix that the tree `t` writes for `univ`
template <typename Plan>
static int record_tree_run(const char *what, st_tree *t, const int64_t *univ, const Plan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed,
                           int32_t stream, st_dispersion_record *out, int64_t *bad_id)
{
    ST_DEVICE(t->device);
    DevBuf<char> d_work;
    DispersionRing ring;
    TwoTreeSession ses(t, t, what);
    const float *d_D = nullptr;
    int rc = dispersion_build_matrix(ses, t, univ, (size_t)P.n_univ, d_D);
    if (rc != ST_OK) return rc;
    rc = record_chunks(d_work, ring, what, ses.s, d_D, P, set_pos, n_pos, seed, stream, out);
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

// a plan of records (record_chunks) over the caller's matrix
template <typename Plan>
static int record_matrix_device(const char *what, int device, const float *D, const Plan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed,
                                int32_t stream, st_dispersion_record *out)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DispersionRing ring;
    DevBuf<float> d_D;
    DrainedStream s;
    if (const int rc = dispersion_upload_matrix(what, D, (size_t)P.n_univ, d_D, s); rc != ST_OK) return rc;
    return record_chunks(d_work, ring, what, s, d_D, P, set_pos, n_pos, seed, stream, out);
}
