// host_swap.h -- part of suchtree_hip.hip (included after host_dispersion.h).  The device side of the swap null:
// st_swap_null_tables (the table rows themselves), st_dispersion_matrix_swap and st_partner_dispersion_swap_host (the
// dispersion records over them).  Kernels: kernels_swap.h (the chains), kernels_dispersion.h (the table form of the three
// task kernels); the plan and the host restatement: swap_plan.cpp.  One work block: the positions, the offsets and row_of,
// then per block of chains their table rows, bit matrices and accepted counts.  The record calls put the live sets and
// two chunks of records behind it and run the chunk loop of the taxa-labels calls (perm_block_chunks_of), whose block
// producer is k_swap_chains here.
#pragma once

// the state of a block of chains inside a work block, and what uploads and launches it
struct SwapDevice {
    size_t o_sets = 0, o_row_of = 0, o_table = 0, o_bits = 0, o_accepted = 0, total = 0;      // (set_pos at 0)
    char *d = nullptr;

    void layout(const SwapPlan &S, int64_t block)
    {
        o_sets = align256((size_t)S.n_pos * 4);
        o_row_of = o_sets + align256((size_t)(S.n_sets + 1) * 8);
        o_table = o_row_of + align256((size_t)S.L * 4);
        o_bits = o_table + align256((size_t)block * (size_t)S.table_bytes);
        o_accepted = o_bits + align256((size_t)block * (size_t)(S.n_sets * S.words) * 8);
        total = o_accepted + align256((size_t)block * 8);
    }
    const int *set_pos() const { return reinterpret_cast<const int *>(d); }
    unsigned short *table() const { return reinterpret_cast<unsigned short *>(d + o_table); }
    long long *accepted() const { return reinterpret_cast<long long *>(d + o_accepted); }
    hipError_t upload(const SwapPlan &S, const int32_t *pos, const int64_t *sets, hipStream_t s) const
    {
        hipError_t e = hipMemcpyAsync(d, pos, (size_t)S.n_pos * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_sets, sets, (size_t)(S.n_sets + 1) * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d + o_row_of, S.row_of.data(), (size_t)S.L * 4, hipMemcpyHostToDevice, s);
        return e;
    }
    // chains p0 .. p0 + n_chains into the block's rows.  For measurements: SUCHTREE_AMD_SWAP_PLAIN=1 takes the plain form, one trial
    // per wave step; SUCHTREE_AMD_SWAP_EARLY=1 the batched form that loads entries and words before the prefix is known
    hipError_t launch(const SwapPlan &S, int64_t p0, int64_t n_chains, uint64_t seed, int32_t stream, hipStream_t s) const
    {
        const SwapChainArgs a{table(),
                              reinterpret_cast<unsigned long long *>(d + o_bits),
                              set_pos(),
                              reinterpret_cast<const long long *>(d + o_sets),
                              reinterpret_cast<const int *>(d + o_row_of),
                              accepted(),
                              (long long)p0,
                              (unsigned long long)seed,
                              (long long)S.iterations,
                              (long long)S.L,
                              (long long)S.e0,
                              (long long)S.n_pos,
                              (long long)S.n_pos,
                              (long long)(S.n_sets * S.words),
                              (long long)n_chains,
                              (int)stream,
                              (int)S.n_sets,
                              (int)S.words};
        auto on = [](const char *name) {
            const char *v = getenv(name);
            return v && v[0] == '1';
        };
        const dim3 grid((unsigned)((n_chains + kSwapThreads / 64 - 1) / (kSwapThreads / 64)));
        if (on("SUCHTREE_AMD_SWAP_PLAIN")) hipLaunchKernelGGL((k_swap_chains<1, false>), grid, dim3(kSwapThreads), 0, s, a);
        else if (on("SUCHTREE_AMD_SWAP_EARLY")) hipLaunchKernelGGL((k_swap_chains<kSwapBatch, true>), grid, dim3(kSwapThreads), 0, s, a);
        else hipLaunchKernelGGL((k_swap_chains<kSwapBatch, false>), grid, dim3(kSwapThreads), 0, s, a);
        return hipGetLastError();
    }
};

static int swap_nomem(const char *what, size_t total, hipError_t e)
{
    (void)hipGetLastError();
    return fail(ST_ERR_NOMEM, std::string(what) + ": a work block of " + std::to_string(total) + " bytes: " + hipGetErrorString(e));
}

// table rows p_begin .. p_begin + n_perms and their accepted counts, block by block of chains
static int swap_tables_device(int device, const SwapPlan &S, const int32_t *set_pos, const int64_t *sets, int64_t p_begin, int64_t n_perms, uint64_t seed,
                              int32_t stream, uint16_t *out, int64_t *accepted)
{
    const char *what = "swap null tables";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DrainedStream s;
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    const int64_t block = swap_block(S, n_perms, 0);
    SwapDevice dev;
    dev.layout(S, block);
    hipError_t e = s.create();
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    e = d_work.alloc(dev.total);
    if (e != hipSuccess) return swap_nomem(what, dev.total, e);
    dev.d = d_work;
    e = dev.upload(S, set_pos, sets, s);
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    for (int64_t b = 0; b < n_perms; b += block) {
        const int64_t n = std::min(block, n_perms - b);
        e = dev.launch(S, p_begin + b, n, seed, stream, s);
        if (e == hipSuccess && S.n_pos > 0) e = hipMemcpyAsync(out + b * S.n_pos, dev.table(), (size_t)n * (size_t)S.table_bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && accepted) e = hipMemcpyAsync(accepted + b, dev.accepted(), (size_t)n * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the next block's chains overwrite the rows)
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    return ST_OK;
}

// the swap-null dispersion call's chunks on stream s over the device matrix d_D: the chains of a block of permutations,
// then the table form of the three task kernels over their rows
static int swap_record_chunks(DevBuf<char> &d_work, DispersionRing &ring, const char *what, hipStream_t s, const float *d_D, const DispersionPlan &P,
                              const SwapPlan &S, const int32_t *set_pos, const int64_t *sets, uint64_t seed, int32_t stream, st_dispersion_record *out,
                              int64_t *accepted)
{
    SwapDevice dev;
    dev.layout(S, P.perm_block);
    const size_t live = P.sets.size(), o_live = dev.total, o_rec = o_live + align256(live * sizeof(DispersionSetDev));
    const size_t rec_bytes = align256((size_t)P.max_chunk_tasks * sizeof(st_dispersion_record)), total = o_rec + 2 * rec_bytes;
    if (const int rc = alloc_work(d_work, total, ring, (size_t)P.max_chunk_tasks, what); rc != ST_OK) return rc;
    std::fill_n(out, P.n_sets * P.rows, st_dispersion_record{0.0, 0.0});      // (every allocation has succeeded: from here on out is written)
    char *const d = d_work;
    dev.d = d;
    st_dispersion_record *const d_rec[2] = {reinterpret_cast<st_dispersion_record *>(d + o_rec),
                                            reinterpret_cast<st_dispersion_record *>(d + o_rec + rec_bytes)};
    hipError_t e = dev.upload(S, set_pos, sets, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_live, P.sets.data(), live * sizeof(DispersionSetDev), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string(what) + " setup: " + hipGetErrorString(e));
    return perm_block_chunks_of(
        ring, what, s, P.chunks, d_rec,
        [&](const DispersionChunk &c, hipStream_t st) {
            hipError_t e1 = dev.launch(S, c.p_begin, c.n_perms, seed, stream, st);
            if (e1 == hipSuccess && accepted)
                e1 = hipMemcpyAsync(accepted + c.p_begin, dev.accepted(), (size_t)c.n_perms * 8, hipMemcpyDeviceToHost, st);
            if (e1 == hipSuccess && accepted) e1 = hipStreamSynchronize(st);      // (the next block's chains overwrite the counts)
            return e1;
        },
        [&](const DispersionChunk &c, st_dispersion_record *d_out, hipStream_t st) {
            DispersionTaskArgs a{d_D, dev.table(), dev.set_pos(), reinterpret_cast<const DispersionSetDev *>(d + o_live), d_out, 0, 0, 0, (unsigned)c.n_perms,
                                 P.n_univ, 0, (int)S.n_pos};
            return dispersion_launch_tasks(
                P.class_begin, c, a, &DispersionTaskArgs::set0, k_swap_tasks_packed, k_swap_tasks_wave, k_swap_tasks_group,
                [&](size_t &lds) {
                    lds = (((size_t)P.max_count + 7) & ~(size_t)7) * 2;
                    return hipSuccess;
                },
                st);
        },
        [&](const st_dispersion_record *records, const DispersionChunk &c) { dispersion_scatter(P, c, records, out); });
}

// the accepted counts of a record call that launches no task (no set of two positions): its chains still run
static void swap_accepted_host(const SwapPlan &S, const int32_t *set_pos, const int64_t *sets, int64_t rows, uint64_t seed, int32_t stream, int64_t *accepted)
{
    std::vector<uint16_t> row((size_t)std::max<int64_t>(S.n_pos, 1));
    for (int64_t p = 0; accepted && p < rows; p++) swap_chain_host(S, set_pos, sets, seed, stream, p, row.data(), accepted + p);
}

static int swap_record_tree_run(const char *what, st_tree *t, const int64_t *univ, const DispersionPlan &P, const SwapPlan &S, const int32_t *set_pos,
                                const int64_t *sets, uint64_t seed, int32_t stream, st_dispersion_record *out, int64_t *accepted, int64_t *bad_id)
{
    ST_DEVICE(t->device);
    DevBuf<char> d_work;
    DispersionRing ring;
    TwoTreeSession ses(t, t, what);
    const float *d_D = nullptr;
    int rc = dispersion_build_matrix(ses, t, univ, (size_t)P.n_univ, d_D);
    if (rc != ST_OK) return rc;
    rc = swap_record_chunks(d_work, ring, what, ses.s, d_D, P, S, set_pos, sets, seed, stream, out, accepted);
    if (rc != ST_OK) return rc;
    return ses.close(bad_id);
}

static int swap_record_matrix_device(const char *what, int device, const float *D, const DispersionPlan &P, const SwapPlan &S, const int32_t *set_pos,
                                     const int64_t *sets, uint64_t seed, int32_t stream, st_dispersion_record *out, int64_t *accepted)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d_work;
    DispersionRing ring;
    DevBuf<float> d_D;
    DrainedStream s;
    if (const int rc = dispersion_upload_matrix(what, D, (size_t)P.n_univ, d_D, s); rc != ST_OK) return rc;
    return swap_record_chunks(d_work, ring, what, s, d_D, P, S, set_pos, sets, seed, stream, out, accepted);
}
