// host_setpair.h -- part of suchtree_hip.hip (included after host_dispersion.h).  The device side of
// st_beta_dispersion_host and st_beta_dispersion_matrix (kernels_setpair.h; the plan, the host restatement and the
// scatter: setpair_plan.cpp).  Everything but the task launches is host_dispersion.h's: the matrix D (built over a SrcGrid
// or uploaded), the work block, the sigma sorts per block of permutations, the chunk loop and its read-back ring
// (dispersion_chunks, with the live directions as its table).
#pragma once

// the launches of tasks [c.task_begin, c.task_begin + c.n_tasks): one per size class whose range of tasks meets the chunk
static hipError_t setpair_launch_tasks(const SetpairPlan &P, const DispersionChunk &c, SetpairTaskArgs a, hipStream_t s)
{
    st_dispersion_record *const rec = a.out;      // the chunk's records: entry t - c.task_begin

    const int64_t lo = c.task_begin, hi = c.task_begin + c.n_tasks, per = kDispersionThreads / 64;
    for (int k = 0; k < kDispersionClasses; k++) {
        const int64_t b = std::max(lo, P.class_begin[k] * c.n_perms), e = std::min(hi, P.class_begin[k + 1] * c.n_perms);
        if (e <= b) continue;
        a.task0 = b / c.n_perms;
        a.perm0 = (unsigned)(b - a.task0 * c.n_perms);
        a.n = e - b;
        a.out = rec + (b - lo);
        a.lanes = 2 << k;
        if (a.lanes <= kDispersionPackedMax) {
            const int64_t waves = (a.n + 64 / a.lanes - 1) / (64 / a.lanes);
            hipLaunchKernelGGL(k_setpair_tasks_packed, dim3((unsigned)((waves + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else if (k == 5) {
            hipLaunchKernelGGL(k_setpair_tasks_wave, dim3((unsigned)((a.n + per - 1) / per)), dim3(kDispersionThreads), 0, s, a);
        } else {
            const size_t lds = setpair_lds_bytes(P.max_walk, P.exclude != 0);      // (up to 64 KiB: above 32 KiB they are asked for)
            const hipError_t e1 = perm_lds_opt_in(k_setpair_tasks_group, lds);
            if (e1 != hipSuccess) return e1;
            hipLaunchKernelGGL(k_setpair_tasks_group, dim3((unsigned)a.n), dim3(kDispersionThreads), lds, s, a);
        }
        const hipError_t e2 = hipGetLastError();
        if (e2 != hipSuccess) return e2;
    }
    return hipSuccess;
}

static int setpair_run_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const float *d_D, const SetpairPlan &P,
                              const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream, st_dispersion_record *out)
{
    return dispersion_chunks(
        d_work, ring, what, s, P, P.tasks, set_pos, n_pos, seed, stream, out, 2 * P.count * P.rows,
        [&](const DispersionChunk &c, const unsigned short *sigma, const int *pos, const SetpairTaskDev *tasks, st_dispersion_record *d_out, hipStream_t st) {
            return setpair_launch_tasks(P, c, SetpairTaskArgs{d_D, sigma, pos, tasks, d_out, 0, 0, 0, (unsigned)c.n_perms, P.n_univ, 0, P.exclude}, st);
        },
        [&](const st_dispersion_record *records, const DispersionChunk &c) { setpair_scatter(P, c, records, out); });
}

static int setpair_run(st_tree *t, const int64_t *univ, const SetpairPlan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream,
                       st_dispersion_record *out, int64_t *bad_id)
{
    ST_DEVICE(t->device);
    DevBuf<char> d_work;
    DispersionRing ring;
    TwoTreeSession ses(t, t, "beta dispersion");
    const float *d_D = nullptr;
    int rc = dispersion_build_matrix(ses, t, univ, (size_t)P.n_univ, d_D);
    if (rc != ST_OK) return rc;
    rc = setpair_run_chunks(d_work, ring, "beta dispersion", ses.s, d_D, P, set_pos, n_pos, seed, stream, out);
    if (rc != ST_OK) return rc;
    return ses.close(bad_id);
}

static int setpair_matrix_device(int device, const float *D, const SetpairPlan &P, const int32_t *set_pos, int64_t n_pos, uint64_t seed, int32_t stream,
                                 st_dispersion_record *out)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DispersionRing ring;
    DevBuf<float> d_D;
    DrainedStream s;
    if (const int rc = dispersion_upload_matrix("beta dispersion matrix", D, (size_t)P.n_univ, d_D, s); rc != ST_OK) return rc;
    return setpair_run_chunks(d_work, ring, "beta dispersion matrix", s, d_D, P, set_pos, n_pos, seed, stream, out);
}
