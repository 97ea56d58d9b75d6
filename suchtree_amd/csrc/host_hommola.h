// host_hommola.h -- part of suchtree_hip.hip (included after host_compare.h).  The device side of
// st_hommola_clades_host and st_hommola_permutation (kernels_hommola.h, kernels_perm.h; the plan and the fold:
// hommola_plan.cpp).  One device block: the float32 matrices -- the other tree's n_o x n_o, then one square per maximal
// clade range, each written once by the unchanged distance kernels over a SrcGrid -- the universes' ids, the links'
// positions, the clade table, one chunk of relabelled positions and two chunks of pieces.  Per chunk of whole blocks:
// the sorts of its rows (k_hommola_relabel*), its blocks (k_hommola_blocks), its pieces copied to one of two pinned
// buffers (ReadbackRing, host_compare.h), folded into their rows while the device works on the next chunk.
#pragma once

// the sorts of one side and size class over a chunk's rows; max_n: the largest universe the class meets in this call
static hipError_t hommola_launch_relabel(const HommolaRelabelArgs &a, int max_n, hipStream_t s)
{
    if (a.cls == kPermSortWave) {
        hipLaunchKernelGGL(k_hommola_relabel_wave, dim3((unsigned)((a.n_rows + 3) / 4)), dim3(256), 0, s, a);
    } else if (a.cls == kPermSortSmall) {
        hipLaunchKernelGGL(k_hommola_relabel<kPermSmallThreads>, dim3((unsigned)a.n_rows), dim3(kPermSmallThreads),
                           perm_lds_bytes(std::min(max_n, kPermSmallMax)), s, a);
    } else {
        hipLaunchKernelGGL(k_hommola_relabel<kPermLargeThreads>, dim3((unsigned)a.n_rows), dim3(kPermLargeThreads), perm_lds_bytes(max_n),
                           s, a);
    }
    return hipGetLastError();
}

static int hommola_clades_run(st_tree *to, st_tree *tc, const int64_t *univ_o, const int64_t *univ_c, const int32_t *pos_o,
                              const int32_t *pos_c, int64_t n_links, const HommolaPlan &P, uint64_t seed, st_pair_moments *out, int64_t *bad_id)
{
    ST_DEVICE(to->device);
    ReadbackRing<CladePiece, BlockSpan> ring;
    TwoTreeSession ses(to, tc, "hommola clades");
    const size_t n_o = (size_t)P.n_univ_o, n_c = (size_t)P.n_univ_c, L = (size_t)n_links;
    const size_t o_uo = align256((size_t)P.mat_floats * 4), o_uc = o_uo + align256(n_o * 8), o_po = o_uc + align256(n_c * 8);
    const size_t o_pc = o_po + align256(L * 4), o_clade = o_pc + align256(L * 4);
    const size_t o_rel = o_clade + align256(P.clades.size() * sizeof(HommolaCladeDev));
    const size_t piece_bytes = align256((size_t)P.max_chunk_blocks * sizeof(CladePiece));
    const size_t o_piece = o_rel + align256((size_t)P.max_chunk_rel * 4), total = o_piece + 2 * piece_bytes;
    int rc = ses.open_or_nomem(total, "one device block", " (" + std::to_string((size_t)P.mat_floats * 4) + " of distance matrices)");
    if (rc != ST_OK) return rc;
    char *const d = ses.d;
    const hipStream_t s = ses.s;
    float *d_mat = reinterpret_cast<float *>(d);
    long long *d_uo = reinterpret_cast<long long *>(d + o_uo), *d_uc = reinterpret_cast<long long *>(d + o_uc);
    const HommolaCladeDev *d_clade = reinterpret_cast<const HommolaCladeDev *>(d + o_clade);
    CladePiece *d_pieces[2] = {reinterpret_cast<CladePiece *>(d + o_piece), reinterpret_cast<CladePiece *>(d + o_piece + piece_bytes)};
    rc = ring.alloc((size_t)P.max_chunk_blocks, ses.what);
    if (rc != ST_OK) return rc;
    hipError_t e = hipMemcpyAsync(d_uo, univ_o, n_o * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_uc, univ_c, n_c * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_po, pos_o, L * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_pc, pos_c, L * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_clade, P.clades.data(), P.clades.size() * sizeof(HommolaCladeDev), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    rc = ses.arm();
    if (rc != ST_OK) return rc;
    // the matrices: D[p][q] = dist(u[p], u[q]), the arguments in that order (not symmetric in the last bit)
    rc = enqueue_grid_dist(to, d_uo, d_uo, n_o, n_o * n_o, d_mat, s);
    for (size_t r = 0; r < P.ranges.size() && rc == ST_OK; r++) {
        const HommolaRange &g = P.ranges[r];
        rc = enqueue_grid_dist(tc, d_uc + g.leaf_begin, d_uc + g.leaf_begin, (size_t)g.leaf_count, (size_t)g.leaf_count * g.leaf_count,
                               d_mat + g.mat_off, s);
    }
    if (rc != ST_OK) return rc;
    int max_leaves = 1;
    for (int64_t c = 0; c < P.n_clades; c++)
        if (P.clades[(size_t)c].link_count >= 2) max_leaves = std::max(max_leaves, P.clades[(size_t)c].leaf_count);
    const size_t lds_large = std::max(perm_lds_bytes(max_leaves), perm_lds_bytes((int)n_o));
    e = perm_lds_opt_in(k_hommola_relabel<kPermLargeThreads>, lds_large);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    auto fold = [&](const CladePiece *pieces, const BlockSpan &b) { hommola_fold(P, b.first, b.count, pieces, out); };
    for (const HommolaChunk &ch : P.chunks) {
        e = ring.acquire(fold);      // (the pieces of two chunks ago)
        if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
        CladePiece *const d_out = d_pieces[ring.next];
        HommolaRelabelArgs ra{d_clade, reinterpret_cast<const int *>(d + o_po), reinterpret_cast<unsigned short *>(d + o_rel), (long long)ch.row_begin,
                              (long long)ch.n_rows, (long long)P.rows_per_clade, (long long)ch.rel_begin, (unsigned long long)seed, 1, (int)n_o,
                              perm_sort_class((int)n_o)};
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
            hipLaunchKernelGGL(k_hommola_blocks, dim3((unsigned)((waves + per - 1) / per)), dim3(kHommolaBlockThreads), 0, s, ba, d_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = ring.post(d_out, (size_t)ch.n_blocks, BlockSpan{ch.block_begin, ch.n_blocks}, s);
        if (e != hipSuccess) return ses.hip_fail(" launch: ", e);
    }
    e = ring.drain(fold, s);
    if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    return ses.close(bad_id);
}

static int hommola_permutation_device(int device, uint64_t seed, int32_t node, int64_t p, int side, int32_t n, int32_t *out)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<int> d_out;
    DrainedStream s;      // (also on an error: the buffer dies behind the kernel)
    hipError_t e = s.create();
    if (e == hipSuccess) e = d_out.alloc((size_t)n);
    const size_t lds = perm_lds_bytes(n);
    if (e == hipSuccess) e = perm_lds_opt_in(k_hommola_permutation<kPermLargeThreads>, lds);      // (above 32 KiB: the large class)
    if (e == hipSuccess) {
        const int cls = perm_sort_class(n);
        if (cls == kPermSortWave) {
            hipLaunchKernelGGL(k_hommola_permutation_wave, dim3(1), dim3(64), 0, s, (unsigned long long)seed, (int)node, (long long)p, side, (int)n, d_out.get());
        } else if (cls == kPermSortSmall) {
            hipLaunchKernelGGL(k_hommola_permutation<kPermSmallThreads>, dim3(1), dim3(kPermSmallThreads), lds, s, (unsigned long long)seed, (int)node,
                               (long long)p, side, (int)n, d_out.get());
        } else {
            hipLaunchKernelGGL(k_hommola_permutation<kPermLargeThreads>, dim3(1), dim3(kPermLargeThreads), lds, s, (unsigned long long)seed,
                               (int)node, (long long)p, side, (int)n, d_out.get());
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("hommola permutation: ") + hipGetErrorString(e));
    return ST_OK;
}
