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

// st_quartets_host: one tree's topologies of n > 0 explicit quartets from and to host arrays, through the slots of the
// tree's own pipe (host_pipe.h).  Its drain copies topologies where run_pipe's unpacks distances and ids, and a chunk is
// packed, uploaded and launched in one step, so the loop is its own; the way out on an error is run_pipe's (pipe_bail).
static int quartets_host_run(st_tree *t, const int64_t *quartets, int64_t n, int64_t stride0, int64_t stride1, int64_t *out_topologies,
                             int64_t *bad_id)
{
    ST_DEVICE(t->device);
    std::lock_guard<std::mutex> lock(t->dp->m);
    HostPipe &pipe = t->dp->pipe;
    // (n,4) int64 in and out are each the size of two pair rows.  Every slot of the pipe carries
    // one chunk: its pinned buffer holds the chunk's quartets (first half) and, later, its
    // topologies (second half, written by the kernel); while chunk c is on the GPU the host
    // unpacks chunk c-2 and packs chunk c+1.
    const int64_t chunk = std::min<int64_t>(n, kHostChunk / 8);
    {
        hipError_t e = pipe.ensure(std::max<int64_t>(4 * chunk, 1024));
        if (e == hipSuccess) e = pipe.ensure_device_in();
        if (e != hipSuccess) return fail(ST_ERR_HIP, std::string("host staging allocation: ") + hipGetErrorString(e));
    }
    if (begin_host_faults(t, pipe.slot[0].stream) != ST_OK) return ST_ERR_HIP;
    const bool canopy = t->strategy == ST_STRATEGY_CANOPY && 6 * chunk >= canopy_min_pairs(t);
    if (canopy && t->q_tmp_cap < kPipeSlots * chunk) {      // six MRCA ids per quartet, per slot
        t->q_tmp_cap = 0;
        ST_HIP(t->q_tmp.alloc((size_t)kPipeSlots * (size_t)chunk * 6));
        t->q_tmp_cap = kPipeSlots * chunk;
    }
    auto out_of = [&](PipeSlot &s) { return reinterpret_cast<int64_t *>(static_cast<char *>(s.h_in) + (size_t)chunk * 32); };
    auto drain = [&](PipeSlot &s) -> hipError_t {
        if (!s.busy) return hipSuccess;
        s.busy = false;
        const hipError_t e = hipEventSynchronize(s.done);
        if (e != hipSuccess) return e;
        pipe.pool.copy(out_topologies + s.off * 4, out_of(s), s.m * 32);     // topologies were written straight into pinned memory
        return hipSuccess;
    };
    int64_t k = 0;
    for (int64_t off = 0; off < n; off += chunk, k++) {
        const int64_t m = std::min(chunk, n - off);
        const int slot_index = (int)(k % kPipeSlots);
        PipeSlot &s = pipe.slot[slot_index];
        hipError_t e = drain(s);
        if (e != hipSuccess) return pipe_bail(pipe, ST_ERR_HIP, std::string("quartet pipeline: ") + hipGetErrorString(e));
        int64_t *h = static_cast<int64_t *>(s.h_in);
        const int64_t *src = quartets + off * stride0;
        pipe.pool.parallel_for(m, [=](int64_t b, int64_t e2) {
            for (int64_t q = b; q < e2; q++)
                for (int c = 0; c < 4; c++) h[4 * q + c] = src[q * stride0 + c * stride1];
        });
        e = hipMemcpyAsync(s.d_in, s.h_in, (size_t)m * 32, hipMemcpyHostToDevice, s.stream);
        if (e != hipSuccess) return pipe_bail(pipe, ST_ERR_HIP, std::string("quartet pipeline: ") + hipGetErrorString(e));
        if (canopy && 6 * m >= canopy_min_pairs(t)) {
            // six MRCA ids per quartet out of the canopy / rank-table kernels, then the pick
            int32_t *tmp = t->q_tmp + (size_t)slot_index * (size_t)chunk * 6;
            const int rc = enqueue_src(t, SrcQuartet{static_cast<const long long *>(s.d_in)}, 6 * m,
                                       DistSink{nullptr, nullptr}, MrcaSink{tmp, nullptr}, t->d_fault_host, s.stream);
            if (rc != ST_OK) return pipe_bail(pipe, rc, g_last_error);
            e = launch_quartet_pick(t, static_cast<const long long *>(s.d_in), static_cast<const int *>(tmp), m,
                                    reinterpret_cast<long long *>(out_of(s)), s.stream);
        } else {
            e = launch_quartets_walk(t, static_cast<const long long *>(s.d_in), m, reinterpret_cast<long long *>(out_of(s)),
                                     t->d_fault_host, s.stream);
        }
        if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
        if (e != hipSuccess) return pipe_bail(pipe, ST_ERR_HIP, std::string("quartet pipeline: ") + hipGetErrorString(e));
        s.busy = true;
        s.off = off;
        s.m = m;
        e = drain(pipe.slot[(k + 1) % kPipeSlots]);      // the oldest chunk, while the newer ones are in flight
        if (e != hipSuccess) return pipe_bail(pipe, ST_ERR_HIP, std::string("quartet pipeline: ") + hipGetErrorString(e));
    }
    for (int j = 0; j < kPipeSlots; j++) {
        const hipError_t e = drain(pipe.slot[(k + j) % kPipeSlots]);
        if (e != hipSuccess) return pipe_bail(pipe, ST_ERR_HIP, std::string("quartet pipeline: ") + hipGetErrorString(e));
    }
    Fault f;
    const int rc = end_host_faults(t, pipe.slot[0].stream, f);
    if (rc != ST_OK) return rc;
    return report_fault(t->n_nodes, f, bad_id);
}
