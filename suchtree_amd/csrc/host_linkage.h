// host_linkage.h -- part of suchtree_hip.hip (included after host_dispersion.h, whose open_work_block it uses).  The
// device side of st_linkage_codes (kernels_linkage.h; the checks and the host restatement: linkage_plan.cpp).  One work
// block: the codes and the weights as uploaded, the square S (rows of linkage_row_stride(n)), the cache and the ids, the
// rows.  Three launches on one stream -- expand, nearest, chain -- and one read-back.
#pragma once

// where the chain keeps its cache: LDS up to kLinkageLdsMaxObjects, else global; the environment variable
// SUCHTREE_AMD_LINKAGE_CACHE = lds / global (read at every call) asks for one, for a test or a measurement: no result
// depends on it, and a cache that does not fit LDS is global whatever is asked
static bool linkage_cache_in_lds(int32_t n)
{
    if (n > kLinkageLdsMaxObjects) return false;
    const char *v = std::getenv("SUCHTREE_AMD_LINKAGE_CACHE");
    return !(v && std::strcmp(v, "global") == 0);
}

static int linkage_device(int device, const int32_t *codes, int32_t n32, const int32_t *weights, int32_t method, st_linkage_row *out)
{
    const char *what = "linkage";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DrainedStream s;
    const size_t n = (size_t)n32, ld = linkage_row_stride(n32), m = n * (n - 1) / 2, out_bytes = (n - 1) * sizeof(st_linkage_row);
    const size_t o_w = align256(m * 4), o_S = o_w + align256(weights ? n * 4 : 0), o_num = o_S + align256(n * ld * 8), o_b = o_num + align256(n * 8);
    const size_t o_size = o_b + align256(n * 4), o_id = o_size + align256(n * 4), o_out = o_id + align256(n * 4), total = o_out + align256(out_bytes);
    if (const int rc = open_work_block(what, s, d_work, total); rc != ST_OK) return rc;
    char *const d = d_work;
    const bool lds = linkage_cache_in_lds(n32);
    const size_t lds_bytes = lds ? n * 16 : 0;
    hipError_t e = hipMemcpyAsync(d, codes, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && weights) e = hipMemcpyAsync(d + o_w, weights, n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && lds) e = perm_lds_opt_in(k_linkage_chain<true>, lds_bytes);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    const int *const d_w = weights ? reinterpret_cast<const int *>(d + o_w) : nullptr;
    const LinkageArgs a{reinterpret_cast<long long *>(d + o_S), reinterpret_cast<long long *>(d + o_num), reinterpret_cast<int *>(d + o_b),
                        reinterpret_cast<int *>(d + o_size), reinterpret_cast<int *>(d + o_id), reinterpret_cast<st_linkage_row *>(d + o_out), (int)n32,
                        (int)method, (unsigned)ld};
    hipLaunchKernelGGL(k_linkage_expand, dim3((unsigned)((n + kLinkageExpandThreads - 1) / kLinkageExpandThreads), (unsigned)n), dim3(kLinkageExpandThreads),
                       0, s, reinterpret_cast<const int *>(d), d_w, a.n, a.method, a.ld, a.S);
    e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_linkage_nearest, dim3((unsigned)n), dim3(kLinkageExpandThreads), 0, s, a.S, d_w, a.n, a.method, a.ld, a.nn_num, a.nn_b, a.size, a.id);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        if (lds)
            hipLaunchKernelGGL(k_linkage_chain<true>, dim3(1), dim3(kLinkageChainThreads), lds_bytes, s, a);
        else
            hipLaunchKernelGGL(k_linkage_chain<false>, dim3(1), dim3(kLinkageChainThreads), 0, s, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    e = hipMemcpyAsync(out, a.out, out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " read-back: " + hipGetErrorString(e));
    return ST_OK;
}
