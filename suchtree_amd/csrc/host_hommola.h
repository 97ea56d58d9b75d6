// host_hommola.h -- part of suchtree_hip.hip (included after host_compare.h).  The device side of
// st_hommola_clades_host and st_hommola_permutation (kernels_hommola.h; the plan, the host form of the permutation and
// the fold: hommola_plan.cpp).  One device block: the float32 matrices -- the other tree's n_o x n_o, then one square per
// maximal clade range, each written once by the unchanged distance kernels over a SrcGrid -- the universes' ids, the
// links' positions, the clade table, one chunk of relabelled positions and two chunks of pieces.  Per chunk of whole
// blocks: the sorts of its rows (k_hommola_relabel*), its blocks (k_hommola_blocks), its pieces copied to one of two
// pinned buffers, folded into their rows while the device works on the next chunk.
#pragma once

static size_t hommola_lds_bytes(int n)
{
    size_t N = 128;
    while (N < (size_t)n) N <<= 1;
    return N * 8;
}

// the sorts of one side and size class over a chunk's rows; max_n: the largest universe the class meets in this call
static hipError_t hommola_launch_relabel(const HommolaRelabelArgs &a, int max_n, hipStream_t s)
{
    if (a.cls == kHommolaSortWave) {
        hipLaunchKernelGGL(k_hommola_relabel_wave, dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, s, a);
    } else if (a.cls == kHommolaSortSmall) {
        hipLaunchKernelGGL(k_hommola_relabel<kHommolaSmallThreads>, dim3((unsigned)a.n_rows), dim3(kHommolaSmallThreads),
                           hommola_lds_bytes(std::min(max_n, kHommolaSmallMax)), s, a);
    } else {
        hipLaunchKernelGGL(k_hommola_relabel<kHommolaLargeThreads>, dim3((unsigned)a.n_rows), dim3(kHommolaLargeThreads), hommola_lds_bytes(max_n),
                           s, a);
    }
    return hipGetLastError();
}

static int hommola_clades_run(st_tree *to, st_tree *tc, const int64_t *univ_o, const int64_t *univ_c, const int32_t *pos_o,
                              const int32_t *pos_c, int64_t n_links, const HommolaPlan &P, uint64_t seed, st_pair_moments *out, int64_t *bad_id)
{
    ST_DEVICE(to->device);
    PinnedBuf<CladePiece> h_pieces[2];      // (declared before the session: they die after its stream has drained)
    Event ev[2];
    TwoTreeSession ses(to, tc, "hommola clades");
    const size_t n_o = (size_t)P.n_univ_o, n_c = (size_t)P.n_univ_c, L = (size_t)n_links;
    const size_t o_uo = align256((size_t)P.mat_floats * 4), o_uc = o_uo + align256(n_o * 8), o_po = o_uc + align256(n_c * 8);
    const size_t o_pc = o_po + align256(L * 4), o_clade = o_pc + align256(L * 4);
    const size_t o_rel = o_clade + align256(P.clades.size() * sizeof(HommolaCladeDev));
    const size_t piece_bytes = align256((size_t)P.max_chunk_blocks * sizeof(CladePiece));
    const size_t o_piece = o_rel + align256((size_t)P.max_chunk_rel * 4), total = o_piece + 2 * piece_bytes;
    hipError_t e = ses.s.create();
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    e = ses.d.alloc(total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ST_ERR_NOMEM, "hommola clades: one device block of " + std::to_string(total) + " bytes (" + std::to_string((size_t)P.mat_floats * 4) +
                                      " of distance matrices): " + hipGetErrorString(e));
    }
    char *const d = ses.d;
    const hipStream_t s = ses.s;
    float *d_mat = reinterpret_cast<float *>(d);
    long long *d_uo = reinterpret_cast<long long *>(d + o_uo), *d_uc = reinterpret_cast<long long *>(d + o_uc);
    const HommolaCladeDev *d_clade = reinterpret_cast<const HommolaCladeDev *>(d + o_clade);
    CladePiece *d_pieces[2] = {reinterpret_cast<CladePiece *>(d + o_piece), reinterpret_cast<CladePiece *>(d + o_piece + piece_bytes)};
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = h_pieces[i].alloc((size_t)P.max_chunk_blocks, hipHostMallocDefault);
        if (e == hipSuccess) e = ev[i].create(hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_uo, univ_o, n_o * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_uc, univ_c, n_c * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_po, pos_o, L * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_pc, pos_c, L * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_clade, P.clades.data(), P.clades.size() * sizeof(HommolaCladeDev), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    int rc = ses.arm();
    if (rc != ST_OK) return rc;
    // the matrices: D[p][q] = dist(u[p], u[q]), the arguments in that order (not symmetric in the last bit)
    rc = enqueue_src(to, SrcGrid{d_uo, d_uo, (long long)n_o, 0, 0}, (int64_t)(n_o * n_o), DistSink{nullptr, d_mat}, MrcaSink{nullptr, nullptr},
                     to->d_fault_host, s);
    for (size_t r = 0; r < P.ranges.size() && rc == ST_OK; r++) {
        const HommolaRange &g = P.ranges[r];
        rc = enqueue_src(tc, SrcGrid{d_uc + g.leaf_begin, d_uc + g.leaf_begin, (long long)g.leaf_count, 0, 0}, (int64_t)g.leaf_count * g.leaf_count,
                         DistSink{nullptr, d_mat + g.mat_off}, MrcaSink{nullptr, nullptr}, tc->d_fault_host, s);
    }
    if (rc != ST_OK) return rc;
    int max_leaves = 1;
    for (int64_t c = 0; c < P.n_clades; c++)
        if (P.clades[(size_t)c].link_count >= 2) max_leaves = std::max(max_leaves, P.clades[(size_t)c].leaf_count);
    const size_t lds_large = std::max(hommola_lds_bytes(max_leaves), hommola_lds_bytes((int)n_o));
    if (lds_large > 32 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_hommola_relabel<kHommolaLargeThreads>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_large);
        if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    }
    int64_t first[2] = {0, 0}, count[2] = {0, 0};
    auto drain = [&](int i) {
        if (count[i] == 0) return hipSuccess;
        const hipError_t de = hipEventSynchronize(ev[i]);
        if (de != hipSuccess) return de;
        hommola_fold(P, first[i], count[i], h_pieces[i], out);
        count[i] = 0;
        return hipSuccess;
    };
    for (size_t k = 0; k < P.chunks.size(); k++) {
        const HommolaChunk &ch = P.chunks[k];
        const int i = (int)(k & 1);
        e = drain(i);      // (the pieces of two chunks ago)
        if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
        HommolaRelabelArgs ra{d_clade, reinterpret_cast<const int *>(d + o_po), reinterpret_cast<unsigned short *>(d + o_rel), (long long)ch.row_begin,
                              (long long)ch.n_rows, (long long)P.rows_per_clade, (long long)ch.rel_begin, (unsigned long long)seed, 1, (int)n_o,
                              hommola_sort_class((int)n_o)};
        e = hommola_launch_relabel(ra, (int)n_o, s);
        ra.pos = reinterpret_cast<const int *>(d + o_pc);
        ra.side = 0;
        for (int cls = 0; cls < 3 && e == hipSuccess; cls++)
            if (ch.side0_classes & (1u << cls)) {
                ra.cls = cls;
                e = hommola_launch_relabel(ra, max_leaves, s);
            }
        if (e == hipSuccess) {
            const HommolaBlockArgs ba{d_clade, d_mat, reinterpret_cast<const unsigned *>(d + o_rel), (long long)ch.block_begin, (long long)ch.n_blocks,
                                      (long long)P.rows_per_clade, (long long)ch.rel_begin, (int)P.n_clades, (int)n_o};
            const int64_t waves = (ch.n_blocks + 63) / 64, per = kHommolaBlockThreads / 64;
            hipLaunchKernelGGL(k_hommola_blocks, dim3((unsigned)((waves + per - 1) / per)), dim3(kHommolaBlockThreads), 0, s, ba, d_pieces[i]);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h_pieces[i], d_pieces[i], (size_t)ch.n_blocks * sizeof(CladePiece), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(ev[i], s);
        if (e != hipSuccess) return ses.hip_fail(" launch: ", e);
        first[i] = ch.block_begin;
        count[i] = ch.n_blocks;
    }
    for (size_t k = P.chunks.size(); k < P.chunks.size() + 2; k++) {      // the older buffer first
        e = drain((int)(k & 1));
        if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    }
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    return ses.close(bad_id);
}

static int hommola_permutation_device(int device, uint64_t seed, int32_t node, int64_t p, int side, int32_t n, int32_t *out)
{
    int n_dev = 0;
    ST_HIP(hipGetDeviceCount(&n_dev));
    if (device >= n_dev) return fail(ST_ERR_ARG, "device " + std::to_string(device) + " of " + std::to_string(n_dev));
    ST_DEVICE(device);
    Stream s;      // (dies after the buffer)
    DevBuf<int> d_out;
    hipError_t e = s.create();
    if (e == hipSuccess) e = d_out.alloc((size_t)n);
    if (e == hipSuccess) {
        const size_t lds = hommola_lds_bytes(n);
        const int cls = hommola_sort_class(n);
        if (cls == kHommolaSortWave) {
            hipLaunchKernelGGL(k_hommola_permutation_wave, dim3(1), dim3(64), 0, s, (unsigned long long)seed, (int)node, (long long)p, side, (int)n, d_out.get());
        } else if (cls == kHommolaSortSmall) {
            hipLaunchKernelGGL(k_hommola_permutation<kHommolaSmallThreads>, dim3(1), dim3(kHommolaSmallThreads), lds, s, (unsigned long long)seed, (int)node,
                               (long long)p, side, (int)n, d_out.get());
        } else {
            if (lds > 32 * 1024)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_hommola_permutation<kHommolaLargeThreads>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds);
            if (e == hipSuccess)
                hipLaunchKernelGGL(k_hommola_permutation<kHommolaLargeThreads>, dim3(1), dim3(kHommolaLargeThreads), lds, s, (unsigned long long)seed,
                                   (int)node, (long long)p, side, (int)n, d_out.get());
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    if (s) {      // (also on an error: the buffer dies behind the kernel)
        const hipError_t es = hipStreamSynchronize(s);
        if (e == hipSuccess) e = es;
    }
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("hommola permutation: ") + hipGetErrorString(e));
    return ST_OK;
}
