// host_parafit.h -- part of suchtree_hip.hip (included after host_dispersion.h, whose work block opener and loop over
// blocks and chunks -- matrix_block_chunks -- it uses).
// The device side of st_parafit_codes (kernels_parafit.h; the plan and the host restatement: parafit_plan.cpp).  One work
// block: g_s and g_f as uploaded, P (row form), the links, one block of R rows, the block's link records, the call's
// totals, the observation's records and the counts.  Once: k_parafit_expand (row form).  Per block of permutations: its
// sorts (k_parafit_relabel*); per chunk of tasks one launch; after a block's last chunk k_parafit_fold.  The totals, the
// observed records and the counts cross the link once, at the end; a block's records cross only where link_all asks.
#pragma once

static hipError_t parafit_launch_relabel(const ParafitRelabelArgs &a, hipStream_t s)
{
    const size_t lds = perm_lds_bytes(a.n_s);
    switch (perm_sort_class(a.n_s)) {
    case kPermSortWave:
        hipLaunchKernelGGL(k_parafit_relabel_wave, dim3((unsigned)((a.n_tasks + 3) / 4)), dim3(256), 0, s, a);
        break;
    case kPermSortSmall:
        hipLaunchKernelGGL(k_parafit_relabel<kPermSmallThreads>, dim3((unsigned)a.n_tasks), dim3(kPermSmallThreads), lds, s, a);
        break;
    default:
        hipLaunchKernelGGL(k_parafit_relabel<kPermLargeThreads>, dim3((unsigned)a.n_tasks), dim3(kPermLargeThreads), lds, s, a);
        break;
    }
    return hipGetLastError();
}

static int parafit_device(int device, const ParafitPlan &P, const int32_t *g_f, const int32_t *g_s, const int32_t *link_f, const int32_t *link_s,
                          uint64_t seed, st_parafit_sum *total, st_parafit_sum *link_obs, int64_t *link_n_ge, st_parafit_sum *link_all)
{
    const char *what = "parafit";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    std::vector<unsigned short> h_lf, h_ls;      // (what the stream's copies read and write: declared before the stream)
    std::vector<ParafitGroupDev> h_group;
    std::vector<ParafitRecord> h_part;
    DevBuf<char> d_work;
    DrainedStream s;
    const size_t n_f = (size_t)P.n_f, n_s = (size_t)P.n_s, L = (size_t)P.n_links, G = P.groups.size();
    const size_t o_gf = align256(n_s * n_s * 4), o_P = o_gf + align256(n_f * n_f * 4), o_lf = o_P + align256(P.wave ? 0 : L * L * 4);
    const size_t o_ls = o_lf + align256(L * 2), o_group = o_ls + align256(L * 2), o_R = o_group + align256(G * sizeof(ParafitGroupDev));
    const size_t o_part = o_R + align256((size_t)P.perm_block * L * 2), o_total = o_part + align256((size_t)P.perm_block * L * sizeof(ParafitRecord));
    const size_t o_obs = o_total + align256((size_t)P.rows * sizeof(st_parafit_sum)), o_nge = o_obs + align256(L * sizeof(st_parafit_sum));
    const size_t bytes = o_nge + align256(L * 8);
    h_lf.resize(L);
    h_ls.resize(L);
    for (size_t l = 0; l < L; l++) {
        h_lf[l] = (unsigned short)link_f[l];
        h_ls[l] = (unsigned short)link_s[l];
    }
    h_group.resize(G);
    for (size_t g = 0; g < G; g++) h_group[g] = ParafitGroupDev{P.groups[g].stream, P.groups[g].begin, P.groups[g].count};
    h_part.resize(link_all ? (size_t)P.perm_block * L : 0);
    if (const int rc = open_work_block(what, s, d_work, bytes); rc != ST_OK) return rc;
    char *const d = d_work;
    const int *const d_gs = reinterpret_cast<const int *>(d), *const d_gf = reinterpret_cast<const int *>(d + o_gf);
    int *const d_P = reinterpret_cast<int *>(d + o_P);
    unsigned short *const d_lf = reinterpret_cast<unsigned short *>(d + o_lf), *const d_ls = reinterpret_cast<unsigned short *>(d + o_ls);
    unsigned short *const d_R = reinterpret_cast<unsigned short *>(d + o_R);
    ParafitGroupDev *const d_group = reinterpret_cast<ParafitGroupDev *>(d + o_group);
    ParafitRecord *const d_part = reinterpret_cast<ParafitRecord *>(d + o_part);
    st_parafit_sum *const d_total = reinterpret_cast<st_parafit_sum *>(d + o_total), *const d_obs = reinterpret_cast<st_parafit_sum *>(d + o_obs);
    long long *const d_nge = reinterpret_cast<long long *>(d + o_nge);
    const size_t row_lds = (n_s * 4 + 15) & ~(size_t)15;
    hipError_t e = hipMemcpyAsync(d, g_s, n_s * n_s * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_gf, g_f, n_f * n_f * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_lf, h_lf.data(), L * 2, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ls, h_ls.data(), L * 2, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_group, h_group.data(), G * sizeof(ParafitGroupDev), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_nge, 0, L * 8, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_parafit_relabel<kPermLargeThreads>, perm_lds_bytes((int)n_s));      // (above 32 KiB: the large class)
    if (e == hipSuccess && !P.wave) e = perm_lds_opt_in(k_parafit_rows, row_lds);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    if (!P.wave) {
        hipLaunchKernelGGL(k_parafit_expand, dim3((unsigned)((L + kParafitThreads - 1) / kParafitThreads), (unsigned)L), dim3(kParafitThreads), 0, s, d_gf,
                           d_lf, (int)n_f, (int)L, d_P);
        if ((e = hipGetLastError()) != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    }
    auto fold = [&](const DispersionChunk &c) {      // the block of chunk c is complete
        const unsigned n_tot = P.wave ? 0u : (unsigned)c.n_perms;
        hipLaunchKernelGGL(k_parafit_fold, dim3(n_tot + (unsigned)L), dim3(64), 0, s, d_part, (int)L, (unsigned)c.n_perms, (long long)c.p_begin,
                           n_tot, d_total + c.p_begin, d_obs, d_nge);
        hipError_t fe = hipGetLastError();
        if (fe != hipSuccess || !link_all) return fe;
        const size_t np = (size_t)c.n_perms;      // (the next block's tasks overwrite the records: they cross now)
        fe = hipMemcpyAsync(h_part.data(), d_part, np * L * sizeof(ParafitRecord), hipMemcpyDeviceToHost, s);
        if (fe == hipSuccess) fe = hipStreamSynchronize(s);
        if (fe != hipSuccess) return fe;
        for (size_t l = 0; l < L; l++)
            for (size_t pb = 0; pb < np; pb++) {
                const ParafitRecord &v = h_part[l * np + pb];
                link_all[((size_t)c.p_begin + pb) * L + l] = st_parafit_sum{v.link_lo, v.link_hi};
            }
        return hipSuccess;
    };
    auto produce = [&](const DispersionChunk &c, hipStream_t st) {      // the block's sorts: R
        return parafit_launch_relabel(ParafitRelabelArgs{d_group, d_ls, d_R, (unsigned long long)seed, (long long)c.p_begin,
                                                         (long long)(c.n_perms * (int64_t)G), (int)G, (int)n_s, (int)L}, st);
    };
    auto launch = [&](const DispersionChunk &c, hipStream_t st) {
        const ParafitArgs a{d_gs, d_P, d_gf, d_lf, d_R, d_part, d_total + c.p_begin, (long long)c.task_begin, (long long)c.n_tasks, (unsigned)c.n_perms,
                            (int)n_f, (int)n_s, (int)L};
        if (P.wave) {
            const int64_t per = kParafitThreads / 64;
            hipLaunchKernelGGL(k_parafit_wave, dim3((unsigned)((a.n_tasks + per - 1) / per)), dim3(kParafitThreads), 0, st, a);
        } else {
            hipLaunchKernelGGL(k_parafit_rows, dim3((unsigned)a.n_tasks), dim3(kParafitThreads), row_lds, st, a);
        }
        return hipGetLastError();
    };
    if (const int rc = matrix_block_chunks(what, s, P.chunks, produce, launch, fold); rc != ST_OK) return rc;
    e = hipMemcpyAsync(total, d_total, (size_t)P.rows * sizeof(st_parafit_sum), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(link_obs, d_obs, L * sizeof(st_parafit_sum), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(link_n_ge, d_nge, L * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " read-back: " + hipGetErrorString(e));
    return ST_OK;
}
