// host_unifrac_null.h -- part of suchtree_hip.hip (included after host_unifrac.h).  The device side of st_unifrac_null_host
// and st_unifrac_null_depths (kernels_unifrac_null.h; the plan, the host restatement and the scatter:
// unifrac_null_plan.cpp).  One work block: the heavy counter, the quantised depths, the range-minimum table, the positions
// and the offsets, one block of sigma rows, its relabelled table, one heavy list and two chunks of int64
// results.  Per block of permutations: its sorts (k_dispersion_sigma); per chunk: the set kernel over its set tasks, the
// lane and wave kernels over its pair tasks (up to three rectangles of pairs x rows), the results copied to one of two
// pinned buffers (ReadbackRing, host_compare.h) and scattered to the caller's arrays while the device works on the next
// chunk.  The head of the block is host_unifrac.h's (UnifracHead), the loop host_dispersion.h's (perm_block_chunks).
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
    hipError_t e = s.create();
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    // the head of host_unifrac.h's block, then this call's: the sigma rows, the relabelled table, the heavy list, the results
    UnifracHead H;
    H.lay_out(P, n_pos, sets);
    const size_t n = (size_t)P.n;
    const size_t o_sigma = H.end, o_rel = o_sigma + align256((size_t)P.perm_block * n * 2);
    const size_t o_heavy = o_rel + align256((size_t)P.perm_block * (size_t)P.n_tab * 2);
    const size_t o_out = o_heavy + align256(P.want_union ? (size_t)P.max_chunk_tasks * 4 : 0);
    const size_t out_bytes = align256((size_t)P.max_chunk_tasks * 8), total = o_out + 2 * out_bytes;
    if (const int rc = alloc_work(d_work, total, ring, (size_t)P.max_chunk_tasks, what); rc != ST_OK) return rc;
    char *const d = d_work;
    e = perm_lds_opt_in(k_dispersion_sigma<kPermLargeThreads>, perm_lds_bytes((int)n));      // (above 32 KiB: the large class)
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    if (const int rc = H.fill(d, what, s, P, d_q, h_q, set_pos, n_pos, sets); rc != ST_OK) return rc;
    const bool heavy = H.heavy;
    int64_t *const d_out[2] = {reinterpret_cast<int64_t *>(d + o_out), reinterpret_cast<int64_t *>(d + o_out + out_bytes)};
    unsigned short *const d_sigma = reinterpret_cast<unsigned short *>(d + o_sigma);
    UnifracNullArgs a{};
    a.d_q = reinterpret_cast<const int64_t *>(d + H.o_dq);
    a.table = reinterpret_cast<const int64_t *>(d + H.o_table);
    a.sigma = d_sigma;
    a.set_pos = reinterpret_cast<const int *>(d + H.o_pos);
    a.sets = reinterpret_cast<const int64_t *>(d + H.o_sets);
    a.relabelled = P.want_union ? reinterpret_cast<unsigned short *>(d + o_rel) : nullptr;
    a.heavy = reinterpret_cast<unsigned *>(d + o_heavy);
    a.n_heavy = reinterpret_cast<unsigned *>(d);
    a.m = P.m;
    a.n_tab = P.n_tab;
    a.n = P.n;
    a.lane_max = H.lane_max;
    a.want_pd = P.want_pd;
    auto launch = [&](const DispersionChunk &c, int64_t *out, hipStream_t) {      // (the stream is s)
        hipError_t e = hipSuccess;
        a.n_perms = (unsigned)c.n_perms;
        // tasks [task_begin, set_end) are set tasks, [set_end, task_begin + n_tasks) pair tasks
        const int64_t end = c.task_begin + c.n_tasks, set_end = std::min(end, std::max(c.task_begin, P.n_sets * c.n_perms));
        if (set_end > c.task_begin) {
            a.task0 = c.task_begin;
            a.count = (unsigned)(set_end - c.task_begin);
            a.out = out;
            hipLaunchKernelGGL(k_null_unifrac_sets, dim3(a.count), dim3(64), 0, s, a);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
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
        return e;
    };
    return perm_block_chunks(ring, what, s, P.chunks, d_sigma, d_out, P.n, seed, stream, launch,
                             [&](const int64_t *got, const DispersionChunk &c) { unifrac_null_scatter(P, c, got, out_pd, out_union); });
}

// the depths of st_unifrac_host (unifrac_tree_depths, host_unifrac.h), then the call above on the tree's device
static int unifrac_null_tree_run(st_tree *t, int64_t root, const int64_t *univ, const UnifracNullPlan &P, const int32_t *set_pos, int64_t n_pos,
                                 const int64_t *sets, int32_t shift, uint64_t seed, int32_t stream, int64_t *out_pd, int64_t *out_union,
                                 int32_t *out_shift, int64_t *bad_id)
{
    UnifracDepths Z;
    {
        ST_DEVICE(t->device);
        TwoTreeSession ses(t, t, "unifrac");
        if (const int rc = unifrac_tree_depths(ses, t, root, univ, P.n, shift, Z, bad_id); rc != ST_OK) return rc;
    }
    if (out_shift) *out_shift = Z.shift;
    if (P.chunks.empty()) return ST_OK;
    return unifrac_null_device(t->device, P, Z.d_q.data(), Z.h_q.data(), set_pos, n_pos, sets, seed, stream, out_pd, out_union);
}
