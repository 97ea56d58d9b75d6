// host_group.h -- part of suchtree_hip.hip (included after host_dispersion.h, whose dispersion_launch_sigma, work block
// opener and loop over blocks and chunks -- matrix_block_chunks -- it uses).  The device side of st_group_sums_codes
// (kernels_group.h; the plan and the host restatement: group_plan.cpp).  One work block: y and the labels as uploaded, one block of sigma rows, the block's
// relabelled labels and partial records (row form), and the call's sums.  Per block of permutations: its sorts
// (k_dispersion_sigma) and, in the row form, its relabel; per chunk of tasks one launch; after a block's last chunk the
// row form's fold.  The sums cross the link once, at the end.  The permutations per task are kGroupSlice, or the
// environment variable SUCHTREE_AMD_GROUP_SLICE = 1 .. 256 (perm_slice_env, read by the export).
#pragma once

static int group_device(int device, const GroupPlan &P, const int32_t *y, const uint8_t *group, uint64_t seed, int32_t stream, int64_t *out)
{
    const char *what = "group sums";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DrainedStream s;
    const size_t n = (size_t)P.n, m = n * (n - 1) / 2, stride = sliced_stride(P.n), out_bytes = (size_t)P.rows * (size_t)P.n_groups * 8;
    const size_t o_group = align256(m * 4), o_sigma = o_group + align256(n), o_G = o_sigma + align256((size_t)P.perm_block * n * 2);
    const size_t o_part = o_G + align256(P.wave ? 0 : (size_t)P.perm_block * stride);
    const size_t o_out = o_part + align256(P.wave ? 0 : (size_t)P.perm_block * n * sizeof(GroupPart));
    const size_t total = o_out + align256(out_bytes);
    if (const int rc = open_work_block(what, s, d_work, total); rc != ST_OK) return rc;
    char *const d = d_work;
    const size_t row_lds = (n * 4 + 15) & ~(size_t)15;
    hipError_t e = hipMemcpyAsync(d, y, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_group, group, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e == hipSuccess && !P.wave) e = perm_lds_opt_in(k_group_rows, row_lds);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    unsigned short *const d_sigma = reinterpret_cast<unsigned short *>(d + o_sigma);
    unsigned char *const d_G = reinterpret_cast<unsigned char *>(d + o_G);
    GroupPart *const d_part = reinterpret_cast<GroupPart *>(d + o_part);
    long long *const d_out = reinterpret_cast<long long *>(d + o_out);
    const unsigned char *const d_group = reinterpret_cast<const unsigned char *>(d + o_group);
    auto fold = [&](const DispersionChunk &c) {      // the block of chunk c is complete
        if (P.wave) return hipSuccess;
        hipLaunchKernelGGL(k_group_fold, dim3((unsigned)c.n_perms), dim3(kGroupThreads), 0, s, d_part, (int)n, (int)P.n_groups,
                           d_out + (size_t)c.p_begin * (size_t)P.n_groups);
        return hipGetLastError();
    };
    auto produce = [&](const DispersionChunk &c, hipStream_t st) {
        hipError_t pe = dispersion_launch_sigma(DispersionSigmaArgs{d_sigma, (long long)c.p_begin, (unsigned long long)seed, (int)stream, (int)n}, c.n_perms, st);
        if (pe != hipSuccess || P.wave) return pe;
        hipLaunchKernelGGL(k_group_relabel, dim3((unsigned)c.n_perms), dim3(kGroupThreads), 0, st, d_sigma, d_group, (int)n, (unsigned)stride, d_G);
        return hipGetLastError();
    };
    auto launch = [&](const DispersionChunk &c, hipStream_t st) {
        if (P.wave) {
            const GroupWaveArgs a{reinterpret_cast<const int *>(d), d_group, d_sigma, d_out + (size_t)c.p_begin * (size_t)P.n_groups, (long long)c.task_begin,
                                  (long long)c.n_tasks, (int)n, (int)P.n_groups};
            const int64_t per = kGroupThreads / 64;
            hipLaunchKernelGGL(k_group_wave, dim3((unsigned)((c.n_tasks + per - 1) / per)), dim3(kGroupThreads), 0, st, a);
        } else {
            const GroupArgs a{reinterpret_cast<const int *>(d), d_G, d_part, (long long)c.task_begin, (unsigned)c.n_perms,
                              (unsigned)dispersion_slices(c.n_perms, P.slice), (unsigned)P.slice, (unsigned)stride, (int)n};
            hipLaunchKernelGGL(k_group_rows, dim3((unsigned)c.n_tasks), dim3(kGroupThreads), row_lds, st, a);
        }
        return hipGetLastError();
    };
    if (const int rc = matrix_block_chunks(what, s, P.chunks, produce, launch, fold); rc != ST_OK) return rc;
    e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " read-back: " + hipGetErrorString(e));
    return ST_OK;
}
