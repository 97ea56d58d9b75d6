// host_quartets.h -- part of suchtree_hip.hip (included after host_compare.h).  The device side of the quartet
// comparison (st_compare_quartets_*_host): quartet_run drives chunks of quartets -- generated on the device from two
// aligned id lists (k_quartet_draw) or uploaded -- through the unchanged MRCA kernels of tree X and then tree Y over
// SrcQuartet (the handle's own policy picks the rank-table, canopy or walk kernel), and k_quartet_agree classifies and
// counts them.  Only the sixteen counts leave the device; device memory is bounded by the chunk: two (c,4) int64 id
// arrays, two 6c int32 MRCA arrays, the table -- and, for generated quartets, the two id lists.  What needs no GPU --
// unranking, the draw, the class rule, argument checks -- is quartet_plan.cpp.
#pragma once

constexpr int64_t kQuartetChunk = (int64_t)1 << 22;      // 2 x 128 MiB of ids + 2 x 96 MiB of MRCA ids

static int quartet_grid(int64_t n) { return (int)std::min<int64_t>((n + kQuartetThreads - 1) / kQuartetThreads, kQuartetBlocks); }

// `count` quartets in chunks of `chunk`: setup(d_extra, stream) stages what every chunk needs in `extra` device bytes
// (the id lists), prep(d_extra, d_qx, d_qy, stream, off, c) fills the two (c,4) id arrays of chunk [off, off + c).
// The locks, the stream, the device block and the fault words are compare_run's: TwoTreeSession (host_compare.h).
template <typename Setup, typename Prep>
static int quartet_run(st_tree *tx, st_tree *ty, int64_t count, int64_t chunk, size_t extra, Setup setup, Prep prep, st_quartet_table *out,
                       int64_t *bad_id)
{
    ST_DEVICE(tx->device);
    TwoTreeSession ses(tx, ty, "quartet compare");
    chunk = std::min(chunk, count);
    // one device block: quartets x | quartets y | MRCA ids x | MRCA ids y | table | caller's data
    const size_t q_bytes = align256((size_t)chunk * 32), m_bytes = align256((size_t)chunk * 24);
    const size_t o_qy = q_bytes, o_mx = 2 * q_bytes, o_my = o_mx + m_bytes, o_table = o_my + m_bytes, o_extra = o_table + 256;
    const size_t total = o_extra + align256(extra);
    int rc = ses.open(total);
    if (rc != ST_OK) return rc;
    char *const d = ses.d;
    const hipStream_t s = ses.s;
    long long *d_qx = reinterpret_cast<long long *>(d), *d_qy = reinterpret_cast<long long *>(d + o_qy);
    int *d_mx = reinterpret_cast<int *>(d + o_mx), *d_my = reinterpret_cast<int *>(d + o_my);
    unsigned long long *d_table = reinterpret_cast<unsigned long long *>(d + o_table);
    char *d_extra = d + o_extra;
    hipError_t e = hipMemsetAsync(d_table, 0, 16 * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = setup(d_extra, s);
    if (e != hipSuccess) return ses.hip_fail(" setup: ", e);
    rc = ses.arm();
    if (rc != ST_OK) return rc;
    for (int64_t off = 0; off < count; off += chunk) {
        const int64_t c = std::min(chunk, count - off);
        e = prep(d_extra, d_qx, d_qy, s, off, c);
        if (e != hipSuccess) return ses.hip_fail(" staging: ", e);
        rc = enqueue_src(tx, SrcQuartet{d_qx}, 6 * c, DistSink{nullptr, nullptr}, MrcaSink{d_mx, nullptr}, tx->d_fault_host, s);
        if (rc == ST_OK) rc = enqueue_src(ty, SrcQuartet{d_qy}, 6 * c, DistSink{nullptr, nullptr}, MrcaSink{d_my, nullptr}, ty->d_fault_host, s);
        if (rc != ST_OK) return rc;
        hipLaunchKernelGGL(k_quartet_agree, dim3(quartet_grid(c)), dim3(kQuartetThreads), 0, s, d_mx, d_my, (long long)c, d_table);
        e = hipGetLastError();
        if (e != hipSuccess) return ses.hip_fail(" launch: ", e);
    }
    unsigned long long cells[16];
    e = hipMemcpyAsync(cells, d_table, sizeof cells, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return ses.hip_fail(" read-back: ", e);
    rc = ses.close(bad_id);
    if (rc != ST_OK) return rc;
    out->n = 0;
    for (int i = 0; i < 16; i++) {
        out->cell[i / 4][i % 4] = (int64_t)cells[i];
        out->n += (int64_t)cells[i];
    }
    if (out->n != count) return fail(ST_ERR_HIP, "quartet compare: counted " + std::to_string(out->n) + " of " + std::to_string(count) + " quartets");
    return ST_OK;
}

template <int MODE>
static hipError_t quartet_draw_launch(const long long *d_ids_x, const long long *d_ids_y, uint64_t seed, int64_t m, int64_t k0, int64_t c,
                                      long long *d_qx, long long *d_qy, int *d_pos, hipStream_t s)
{
    hipLaunchKernelGGL(k_quartet_draw<MODE>, dim3(quartet_grid(c)), dim3(kQuartetThreads), 0, s, d_ids_x, d_ids_y, (unsigned long long)seed,
                       (long long)m, (long long)k0, (long long)c, d_qx, d_qy, d_pos);
    return hipGetLastError();
}

static hipError_t quartet_draw_any(int mode, const long long *d_ids_x, const long long *d_ids_y, uint64_t seed, int64_t m, int64_t k0, int64_t c,
                                   long long *d_qx, long long *d_qy, int *d_pos, hipStream_t s)
{
    return mode == ST_QUARTET_ALL ? quartet_draw_launch<ST_QUARTET_ALL>(d_ids_x, d_ids_y, seed, m, k0, c, d_qx, d_qy, d_pos, s)
                                  : quartet_draw_launch<ST_QUARTET_SAMPLE>(d_ids_x, d_ids_y, seed, m, k0, c, d_qx, d_qy, d_pos, s);
}

// generated quartets over two aligned id lists (arguments checked by the caller)
static int quartet_leaves_run(st_tree *tx, st_tree *ty, const int64_t *ids_x, const int64_t *ids_y, int64_t m, int mode, uint64_t seed,
                              int64_t k_begin, int64_t k_count, int64_t chunk, st_quartet_table *out, int64_t *bad_id)
{
    const size_t list = align256((size_t)m * 8);
    auto setup = [&](char *d_extra, hipStream_t s) {
        hipError_t e = hipMemcpyAsync(d_extra, ids_x, (size_t)m * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_extra + list, ids_y, (size_t)m * 8, hipMemcpyHostToDevice, s);
        return e;
    };
    auto prep = [&](char *d_extra, long long *d_qx, long long *d_qy, hipStream_t s, int64_t off, int64_t c) {
        return quartet_draw_any(mode, reinterpret_cast<const long long *>(d_extra), reinterpret_cast<const long long *>(d_extra + list), seed, m,
                                k_begin + off, c, d_qx, d_qy, nullptr, s);
    };
    return quartet_run(tx, ty, k_count, chunk, 2 * list, setup, prep, out, bad_id);
}

// explicit quartets, uploaded chunk by chunk
static int quartet_given_run(st_tree *tx, st_tree *ty, const int64_t *quartets_x, const int64_t *quartets_y, int64_t n, int64_t chunk,
                             st_quartet_table *out, int64_t *bad_id)
{
    auto setup = [](char *, hipStream_t) { return hipSuccess; };
    auto prep = [&](char *, long long *d_qx, long long *d_qy, hipStream_t s, int64_t off, int64_t c) {
        hipError_t e = hipMemcpyAsync(d_qx, quartets_x + 4 * off, (size_t)c * 32, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_qy, quartets_y + 4 * off, (size_t)c * 32, hipMemcpyHostToDevice, s);
        return e;
    };
    return quartet_run(tx, ty, n, chunk, 0, setup, prep, out, bad_id);
}

// st_quartet_positions on a device: the generator kernel alone, chunk by chunk into one device buffer
static int quartet_positions_device(int device, int mode, uint64_t seed, int64_t m, int64_t k_begin, int64_t k_count, int32_t *out_pos)
{
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    const int64_t chunk = std::min(k_count, kQuartetChunk);
    DevBuf<int> d_pos;
    DrainedStream s;      // (an error may leave the draw kernel running: the buffer dies behind it)
    hipError_t e = s.create();
    if (e == hipSuccess) e = d_pos.alloc((size_t)chunk * 4);
    for (int64_t off = 0; off < k_count && e == hipSuccess; off += chunk) {
        const int64_t c = std::min(chunk, k_count - off);
        e = quartet_draw_any(mode, nullptr, nullptr, seed, m, k_begin + off, c, nullptr, nullptr, d_pos, s);
        if (e == hipSuccess) e = hipMemcpyAsync(out_pos + 4 * off, d_pos, (size_t)c * 16, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // (the buffer is reused by the next chunk)
    }
    if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("quartet positions: ") + hipGetErrorString(e));
    return ST_OK;
}
