// host_rf.h -- part of suchtree_hip.hip (included after host_linkage.h).  The device side of st_rf_tasks (kernels_rf.h; the
// checks, the tables and the host restatement: rf_plan.cpp).  One work block, uploaded once: the positions, the
// alignments, the offsets, the ranges, the sorted keys with their indices, the explicit tasks, the counts and two chunks
// of results.  Per chunk of tasks one launch of k_rf_tasks; its int32 per task is copied to one of two pinned buffers
// (ReadbackRing, host_compare.h) and moved to the caller's array while the device works on the next chunk.  The counts
// are read back once, at the end.
#pragma once

using RfRing = ReadbackRing<int32_t, BlockSpan>;

static int rf_device(int device, const RfPlan &P, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int32_t *out_shared,
                     int64_t *out_count)
{
    const char *what = "rf tasks";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d;      // (declared before the stream's owner)
    RfRing ring;
    DrainedStream s;
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    hipError_t e = s.create();
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    const size_t n_clades = (size_t)P.n_clades, chunk = (size_t)P.chunk, n_explicit = P.triangle ? 0 : (size_t)P.n_tasks;
    const size_t o_align = align256(P.where.size() * 2), o_off = o_align + align256(P.align.size() * 2), o_range = o_off + align256(P.off.size() * 4);
    const size_t o_key = o_range + align256(n_clades * 4), o_idx = o_key + align256(n_clades * 4), o_ti = o_idx + align256(n_clades * 4);
    const size_t o_tj = o_ti + align256(n_explicit * 4), o_tp = o_tj + align256(n_explicit * 4), o_count = o_tp + align256(task_p ? n_explicit * 4 : 0);
    const size_t o_out = o_count + align256(out_count ? n_clades * 8 : 0), out_bytes = align256(chunk * 4), total = o_out + 2 * out_bytes;
    if (const int rc = alloc_work(d, total, ring, chunk, what); rc != ST_OK) return rc;
    char *const base = d;
    auto upload = [&](size_t at, const void *src, size_t bytes) {
        if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, s);
    };
    upload(0, P.where.data(), P.where.size() * 2);
    upload(o_align, P.align.data(), P.align.size() * 2);
    upload(o_off, P.off.data(), P.off.size() * 4);
    upload(o_range, P.range.data(), n_clades * 4);
    upload(o_key, P.key.data(), n_clades * 4);
    upload(o_idx, P.idx.data(), n_clades * 4);
    upload(o_ti, task_i, n_explicit * 4);
    upload(o_tj, task_j, n_explicit * 4);
    if (task_p) upload(o_tp, task_p, n_explicit * 4);
    if (e == hipSuccess && out_count && n_clades > 0) e = hipMemsetAsync(base + o_count, 0, n_clades * 8, s);
    const size_t lds = rf_lds_bytes(P.m);
    if (e == hipSuccess) e = perm_lds_opt_in(k_rf_tasks, lds);
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    int *d_out[2] = {reinterpret_cast<int *>(base + o_out), reinterpret_cast<int *>(base + o_out + out_bytes)};
    auto deliver = [&](const int32_t *got, const BlockSpan &tasks) { std::copy(got, got + tasks.count, out_shared + tasks.first); };
    RfArgs a{};
    a.where = reinterpret_cast<const unsigned short *>(base);
    a.align = reinterpret_cast<const unsigned short *>(base + o_align);
    a.off = reinterpret_cast<const int *>(base + o_off);
    a.range = reinterpret_cast<const unsigned *>(base + o_range);
    a.key = reinterpret_cast<const unsigned *>(base + o_key);
    a.idx = reinterpret_cast<const int *>(base + o_idx);
    a.task_i = P.triangle ? nullptr : reinterpret_cast<const int *>(base + o_ti);
    a.task_j = P.triangle ? nullptr : reinterpret_cast<const int *>(base + o_tj);
    a.task_p = P.triangle || !task_p ? nullptr : reinterpret_cast<const int *>(base + o_tp);
    a.count = out_count ? reinterpret_cast<unsigned long long *>(base + o_count) : nullptr;
    a.m = P.m;
    a.unrooted = P.unrooted ? 1 : 0;
    for (int64_t at = 0; at < P.n_tasks; at += (int64_t)chunk) {
        const int64_t tasks = std::min<int64_t>((int64_t)chunk, P.n_tasks - at);
        e = ring.acquire(deliver);      // (the results of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        a.first = (P.triangle ? P.begin : 0) + at;
        a.out = d_out[ring.next];
        a.tasks = (int)tasks;
        hipLaunchKernelGGL(k_rf_tasks, dim3((unsigned)std::min<int64_t>(tasks, kRfBlocks)), dim3(kRfThreads), lds, s, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = ring.post(a.out, (size_t)tasks, BlockSpan{at, tasks}, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    if (out_count && n_clades > 0) {
        e = hipMemcpyAsync(out_count, base + o_count, n_clades * 8, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
    }
    e = ring.drain(deliver, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}
