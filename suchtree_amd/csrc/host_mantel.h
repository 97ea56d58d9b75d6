// host_mantel.h -- part of suchtree_hip.hip (included after host_dispersion.h, whose dispersion_launch_sigma, work block
// opener and loop over blocks and chunks -- matrix_block_chunks -- it uses).
// The device side of st_mantel_codes (kernels_mantel.h; the plan and the host restatement: mantel_plan.cpp).  One work
// block: x_sq, y and z as uploaded, one block of sigma rows, the block's partial records (row form) and the call's
// records.  Per block of permutations: its sorts (k_dispersion_sigma); per chunk of tasks one launch; after a block's
// last chunk the row form folds its partial records into the block's records.  The records cross the link once, at the end.
#pragma once

// the environment variable SUCHTREE_AMD_MANTEL_GATHER=1 (read at every call) runs the row form's tasks without the LDS
// row, for a measurement: no result depends on it
static bool mantel_gather()
{
    const char *v = std::getenv("SUCHTREE_AMD_MANTEL_GATHER");
    return v && v[0] == '1';
}

template <bool Z>
static hipError_t mantel_launch_chunk(const MantelPlan &P, const MantelArgs &a, size_t row_lds, bool gather, hipStream_t s)
{
    if (P.wave) {
        const int64_t per = kMantelThreads / 64;
        hipLaunchKernelGGL(k_mantel_wave<Z>, dim3((unsigned)((a.n_tasks + per - 1) / per)), dim3(kMantelThreads), 0, s, a);
    } else if (gather) {
        hipLaunchKernelGGL((k_mantel_rows<Z, true>), dim3((unsigned)a.n_tasks), dim3(kMantelThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_mantel_rows<Z, false>), dim3((unsigned)a.n_tasks), dim3(kMantelThreads), row_lds, s, a);
    }
    return hipGetLastError();
}

static int mantel_device(int device, const MantelPlan &P, const int32_t *x_sq, const int32_t *y, const int32_t *z, uint64_t seed, int32_t stream,
                         st_mantel_sums *out)
{
    const char *what = "mantel";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DrainedStream s;
    const size_t n = (size_t)P.n, m = n * (n - 1) / 2;
    const size_t o_y = align256(n * n * 4), o_z = o_y + align256(m * 4), o_sigma = o_z + align256(P.partial ? m * 4 : 0);
    const size_t o_part = o_sigma + align256((size_t)P.perm_block * n * 2);
    const size_t o_out = o_part + align256(P.wave ? 0 : (size_t)(P.items * P.perm_block) * sizeof(st_mantel_sums));
    const size_t total = o_out + align256((size_t)P.rows * sizeof(st_mantel_sums));
    if (const int rc = open_work_block(what, s, d_work, total); rc != ST_OK) return rc;
    char *const d = d_work;
    const size_t row_lds = (n * 4 + 15) & ~(size_t)15;
    hipError_t e = hipMemcpyAsync(d, x_sq, n * n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_y, y, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && P.partial) e = hipMemcpyAsync(d + o_z, z, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    const bool gather = mantel_gather();
    if (e == hipSuccess && !P.wave && !gather)
        e = P.partial ? perm_lds_opt_in(k_mantel_rows<true, false>, row_lds) : perm_lds_opt_in(k_mantel_rows<false, false>, row_lds);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    unsigned short *const d_sigma = reinterpret_cast<unsigned short *>(d + o_sigma);
    st_mantel_sums *const d_part = reinterpret_cast<st_mantel_sums *>(d + o_part), *const d_out = reinterpret_cast<st_mantel_sums *>(d + o_out);
    auto fold = [&](const DispersionChunk &c) {      // the block of chunk c is complete
        if (P.wave) return hipSuccess;
        hipLaunchKernelGGL(k_mantel_fold, dim3((unsigned)c.n_perms), dim3(64), 0, s, d_part, (int)P.items, (unsigned)c.n_perms, d_out + c.p_begin);
        return hipGetLastError();
    };
    auto produce = [&](const DispersionChunk &c, hipStream_t st) {
        return dispersion_launch_sigma(DispersionSigmaArgs{d_sigma, (long long)c.p_begin, (unsigned long long)seed, (int)stream, (int)n}, c.n_perms, st);
    };
    auto launch = [&](const DispersionChunk &c, hipStream_t st) {
        const MantelArgs a{reinterpret_cast<const int *>(d), reinterpret_cast<const int *>(d + o_y), reinterpret_cast<const int *>(d + o_z), d_sigma,
                           P.wave ? d_out + c.p_begin : d_part, (long long)c.task_begin, (long long)c.n_tasks, (unsigned)c.n_perms, (int)n};
        return P.partial ? mantel_launch_chunk<true>(P, a, row_lds, gather, st) : mantel_launch_chunk<false>(P, a, row_lds, gather, st);
    };
    if (const int rc = matrix_block_chunks(what, s, P.chunks, produce, launch, fold); rc != ST_OK) return rc;
    e = hipMemcpyAsync(out, d_out, (size_t)P.rows * sizeof(st_mantel_sums), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " read-back: " + hipGetErrorString(e));
    return ST_OK;
}
