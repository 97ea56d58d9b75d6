// host_unifrac_null.h -- part of suchtree_hip.hip (included after host_unifrac.h).  The device side of st_unifrac_null_host
// and st_unifrac_null_depths (kernels_unifrac_null.h; the plan, the host restatement and the scatter:
// unifrac_null_plan.cpp).  One work block: the heavy counter, the quantised depths, the range-minimum table, the positions
// and the offsets, one block of sigma rows, its relabelled table, one heavy list and two chunks of int64
// results.  Per block of permutations: its sorts (k_dispersion_sigma); per chunk: the set kernel over its set tasks, the
// lane and wave kernels over its pair tasks (up to three rectangles of pairs x rows), the results copied to one of two pinned buffers (ReadbackRing, host_compare.h)
// and scattered to the caller's arrays while the device works on the next chunk.
#pragma once

using UnifracNullRing = ReadbackRing<int64_t, const DispersionChunk *>;

static int unifrac_null_device(int device, const UnifracNullPlan &P, const int64_t *d_q, const int64_t *h_q, const int32_t *set_pos, int64_t n_pos,
                               const int64_t *sets, uint64_t seed, int32_t stream, int64_t *out_pd, int64_t *out_union)
{
    const char *what = "unifrac null";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;      // (declared before the stream's owner)
    UnifracNullRing ring;
    DrainedStream s;
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    hipError_t e = s.create();
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    const size_t n = (size_t)P.n, n_off = (size_t)P.n_sets + 1;
    const size_t o_dq = 256;      // (the counter has the block's first bytes)
    const size_t o_table = o_dq + align256(n * 8), o_pos = o_table + align256((size_t)P.levels * (size_t)P.m * 8);
    const size_t o_sets = o_pos + align256((size_t)n_pos * 4);
    const size_t o_sigma = o_sets + align256(n_off * 8), o_rel = o_sigma + align256((size_t)P.perm_block * n * 2);
    const size_t o_heavy = o_rel + align256((size_t)P.perm_block * (size_t)P.n_tab * 2);
    const size_t o_out = o_heavy + align256(P.want_union ? (size_t)P.max_chunk_tasks * 4 : 0);
    const size_t out_bytes = align256((size_t)P.max_chunk_tasks * 8), total = o_out + 2 * out_bytes;
    if (const int rc = alloc_work(d_work, total, ring, (size_t)P.max_chunk_tasks, what); rc != ST_OK) return rc;
    char *const d = d_work;
    int64_t *const d_table = reinterpret_cast<int64_t *>(d + o_table);
    e = hipMemcpyAsync(d + o_dq, d_q, n * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && P.m > 0) e = hipMemcpyAsync(d_table, h_q, (size_t)P.m * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_pos > 0) e = hipMemcpyAsync(d + o_pos, set_pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_sets, sets, n_off * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    for (int l = 1; l < P.levels; l++) {      // (2^l <= m: every level has an entry)
        const int64_t half = (int64_t)1 << (l - 1), count = P.m - 2 * half + 1;
        hipLaunchKernelGGL(k_unifrac_table, dim3((unsigned)((count + kUnifracThreads - 1) / kUnifracThreads)), dim3(kUnifracThreads), 0, s,
                           d_table + (int64_t)(l - 1) * P.m, d_table + (int64_t)l * P.m, (long long)half, (long long)count);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    int64_t largest = 0;
    for (int64_t r = 0; r < P.n_sets; r++) largest = std::max(largest, sets[r + 1] - sets[r]);
    const int lane_max = unifrac_lane_max();
    const bool heavy = 2 * largest > lane_max;      // (else no task reaches the wave form: its launch is left out)
    int64_t *d_out[2] = {reinterpret_cast<int64_t *>(d + o_out), reinterpret_cast<int64_t *>(d + o_out + out_bytes)};
    auto scatter = [&](const int64_t *got, const DispersionChunk *c) { unifrac_null_scatter(P, *c, got, out_pd, out_union); };
    UnifracNullArgs a{};
    a.d_q = reinterpret_cast<const int64_t *>(d + o_dq);
    a.table = d_table;
    a.sigma = reinterpret_cast<const unsigned short *>(d + o_sigma);
    a.set_pos = reinterpret_cast<const int *>(d + o_pos);
    a.sets = reinterpret_cast<const int64_t *>(d + o_sets);
    a.relabelled = P.want_union ? reinterpret_cast<unsigned short *>(d + o_rel) : nullptr;
    a.heavy = reinterpret_cast<unsigned *>(d + o_heavy);
    a.n_heavy = reinterpret_cast<unsigned *>(d);
    a.m = P.m;
    a.n_tab = P.n_tab;
    a.n = P.n;
    a.lane_max = lane_max;
    a.want_pd = P.want_pd;
    int64_t sigma_p = -1;      // the block whose rows the device holds
    for (const DispersionChunk &c : P.chunks) {
        e = ring.acquire(scatter);      // (the results of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        int64_t *const out = d_out[ring.next];
        if (c.p_begin != sigma_p) {      // (stream order: the tasks of the block before have read their rows)
            e = dispersion_launch_sigma(DispersionSigmaArgs{reinterpret_cast<unsigned short *>(d + o_sigma), (long long)c.p_begin, (unsigned long long)seed,
                                                            (int)stream, (int)n},
                                        c.n_perms, s);
            if (e != hipSuccess) return hip_fail(" launch: ", e);
            sigma_p = c.p_begin;
        }
        a.n_perms = (unsigned)c.n_perms;
        // tasks [task_begin, set_end) are set tasks, [set_end, task_begin + n_tasks) pair tasks
        const int64_t end = c.task_begin + c.n_tasks, set_end = std::min(end, std::max(c.task_begin, P.n_sets * c.n_perms));
        if (set_end > c.task_begin) {
            a.task0 = c.task_begin;
            a.count = (unsigned)(set_end - c.task_begin);
            a.out = out;
            hipLaunchKernelGGL(k_null_unifrac_sets, dim3(a.count), dim3(64), 0, s, a);
            e = hipGetLastError();
            if (e != hipSuccess) return hip_fail(" launch: ", e);
        }
        // the pair tasks as rectangles of pairs x rows, their results at pair * n_perms + row of the chunk's buffer: the rest
        // of a pair the chunk before began, whole pairs, the rows of a last pair the next chunk finishes
        auto pairs = [&](int64_t t, int64_t n_pairs, int64_t count) {
            a.pair_first = P.k_begin + (t / c.n_perms - P.n_sets);
            a.n_pairs = (unsigned)n_pairs;
            a.p_first = (unsigned)(t % c.n_perms);
            a.count = (unsigned)count;
            a.out = out + (t - c.task_begin);
            hipError_t e2 = heavy ? hipMemsetAsync(d, 0, 16, s) : hipSuccess;      // (stream order: the wave kernel before has read it)
            if (e2 != hipSuccess) return e2;
            hipLaunchKernelGGL(k_null_unifrac_lane, dim3((a.count + kUnifracThreads - 1) / kUnifracThreads), dim3(kUnifracThreads), 0, s, a);
            e2 = hipGetLastError();
            if (e2 == hipSuccess && heavy) {
                hipLaunchKernelGGL(k_null_unifrac_wave, dim3(kUnifracWaveBlocks), dim3(kUnifracThreads), 0, s, a);
                e2 = hipGetLastError();
            }
            return e2;
        };
        int64_t t = set_end;
        if (t < end && t % c.n_perms != 0) {
            const int64_t count = std::min(c.n_perms - t % c.n_perms, end - t);
            e = pairs(t, 1, count);
            t += count;
        }
        if (e == hipSuccess && end - t >= c.n_perms) {
            const int64_t whole = (end - t) / c.n_perms;
            e = pairs(t, whole, whole * c.n_perms);
            t += whole * c.n_perms;
        }
        if (e == hipSuccess && t < end) e = pairs(t, 1, end - t);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
        e = ring.post(out, (size_t)c.n_tasks, &c, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    e = ring.drain(scatter, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}

// the depths of st_unifrac_host (unifrac_tree_run with a plan of no chunks: d, h and the shift used), quantised on the
// host by the caller's shift once more (the same rule on the same values), then the call above on the tree's device
static int unifrac_null_tree_run(st_tree *t, int64_t root, const int64_t *univ, const UnifracNullPlan &P, const int32_t *set_pos, int64_t n_pos,
                                 const int64_t *sets, int32_t shift, uint64_t seed, int32_t stream, int64_t *out_pd, int64_t *out_union,
                                 int32_t *out_shift, int64_t *bad_id)
{
    UnifracPlan D;      // the depths alone
    D.n = P.n;
    D.m = P.m;
    D.levels = P.levels;
    D.n_sets = P.n_sets;
    std::vector<float> h_d((size_t)P.n), h_h((size_t)P.m);
    int32_t used = 0;
    int rc = unifrac_tree_run(t, root, univ, D, set_pos, n_pos, sets, shift, nullptr, nullptr, &used, h_d.data(), h_h.data(), bad_id);
    if (rc != ST_OK) return rc;
    if (out_shift) *out_shift = used;
    if (P.chunks.empty()) return ST_OK;
    std::vector<int64_t> d_q((size_t)P.n), h_q((size_t)P.m);
    std::string err;
    rc = unifrac_quantise(h_d.data(), h_h.data(), P.n, shift, d_q.data(), h_q.data(), nullptr, err);
    if (rc != ST_OK) return fail(rc, err);
    return unifrac_null_device(t->device, P, d_q.data(), h_q.data(), set_pos, n_pos, sets, seed, stream, out_pd, out_union);
}
