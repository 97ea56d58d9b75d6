// host_class.h -- part of suchtree_hip.hip (included after host_dispersion.h, whose dispersion_launch_sigma, work block
// opener and loop over blocks and chunks -- matrix_block_chunks -- it uses).  The device side of st_class_sums_codes
// (kernels_class.h; the plan and the host restatement: class_plan.cpp).  One work block: y and the condensed classes
// as uploaded, the class square and the block's partial sums (row form), one block of sigma rows, and the call's sums.
// Once a call the row form's expand; per
// block of permutations its sorts (k_dispersion_sigma); per chunk of tasks one launch; after a block's last chunk the
// row form's fold.  The sums cross the link once, at the end.  The permutations per task are kClassSlice, or the
// environment variable SUCHTREE_AMD_CLASS_SLICE = 1 .. 256 (perm_slice_env, read by the export).
#pragma once

// the environment variable SUCHTREE_AMD_CLASS_ACC = compare (read at every call) runs the row form that was measured
// against the LDS accumulators (kernels_class.h), for a measurement: no result depends on it
static bool class_compare_form()
{
    const char *v = std::getenv("SUCHTREE_AMD_CLASS_ACC");
    return v && std::strcmp(v, "compare") == 0;
}

static int class_device(int device, const ClassPlan &P, const int32_t *y, const uint8_t *cls, uint64_t seed, int32_t stream, int64_t *out)
{
    const char *what = "class sums";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DrainedStream s;
    const size_t n = (size_t)P.n, m = n * (n - 1) / 2, stride = sliced_stride(P.n), K = (size_t)P.n_classes, out_bytes = (size_t)P.rows * K * 8;
    const size_t o_cls = align256(m * 4), o_sq = o_cls + align256(m), o_sigma = o_sq + align256(P.wave ? 0 : n * stride);
    const size_t o_part = o_sigma + align256((size_t)P.perm_block * n * 2);
    const size_t o_out = o_part + align256(P.wave ? 0 : (size_t)P.perm_block * (size_t)P.items * K * 8);
    const size_t total = o_out + align256(out_bytes);
    if (const int rc = open_work_block(what, s, d_work, total); rc != ST_OK) return rc;
    char *const d = d_work;
    const size_t row_lds = class_row_lds(P.n), acc_lds = (kClassThreads / 64) * kClassMax * kClassCopies * 8;      // (the accumulators are static: counted towards the opt-in)
    const bool compare = class_compare_form();
    hipError_t e = hipMemcpyAsync(d, y, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_cls, cls, m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e == hipSuccess && !P.wave) e = compare ? perm_lds_opt_in(k_class_rows<true>, row_lds + acc_lds) : perm_lds_opt_in(k_class_rows<false>, row_lds + acc_lds);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    const unsigned char *const d_cls = reinterpret_cast<const unsigned char *>(d + o_cls);
    unsigned char *const d_sq = reinterpret_cast<unsigned char *>(d + o_sq);
    unsigned short *const d_sigma = reinterpret_cast<unsigned short *>(d + o_sigma);
    long long *const d_part = reinterpret_cast<long long *>(d + o_part);
    long long *const d_out = reinterpret_cast<long long *>(d + o_out);
    if (!P.wave) {
        hipLaunchKernelGGL(k_class_expand, dim3((unsigned)((stride + kClassThreads - 1) / kClassThreads), (unsigned)n), dim3(kClassThreads), 0, s, d_cls,
                           (int)n, (unsigned)stride, d_sq);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    }
    auto fold = [&](const DispersionChunk &c) {      // the block of chunk c is complete
        if (P.wave) return hipSuccess;
        hipLaunchKernelGGL(k_class_fold, dim3((unsigned)c.n_perms), dim3(kClassThreads), 0, s, d_part, (int)P.items, (int)K, d_out + (size_t)c.p_begin * K);
        return hipGetLastError();
    };
    auto produce = [&](const DispersionChunk &c, hipStream_t st) {
        return dispersion_launch_sigma(DispersionSigmaArgs{d_sigma, (long long)c.p_begin, (unsigned long long)seed, (int)stream, (int)n}, c.n_perms, st);
    };
    auto launch = [&](const DispersionChunk &c, hipStream_t st) {
        if (P.wave) {
            const ClassWaveArgs a{reinterpret_cast<const int *>(d), d_cls, d_sigma, d_out + (size_t)c.p_begin * K, (long long)c.task_begin, (long long)c.n_tasks,
                                  (int)n, (int)K};
            const int64_t per = kClassThreads / 64;
            hipLaunchKernelGGL(k_class_wave, dim3((unsigned)((c.n_tasks + per - 1) / per)), dim3(kClassThreads), 0, st, a);
        } else {
            const ClassArgs a{reinterpret_cast<const int *>(d), d_sq, d_sigma, d_part, (long long)c.task_begin, (unsigned)c.n_perms,
                              (unsigned)dispersion_slices(c.n_perms, P.slice), (unsigned)P.slice, (unsigned)stride, (int)n, (int)K, (int)P.items};
            if (compare)
                hipLaunchKernelGGL(k_class_rows<true>, dim3((unsigned)c.n_tasks), dim3(kClassThreads), row_lds, st, a);
            else
                hipLaunchKernelGGL(k_class_rows<false>, dim3((unsigned)c.n_tasks), dim3(kClassThreads), row_lds, st, a);
        }
        return hipGetLastError();
    };
    if (const int rc = matrix_block_chunks(what, s, P.chunks, produce, launch, fold); rc != ST_OK) return rc;
    e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " read-back: " + hipGetErrorString(e));
    return ST_OK;
}
