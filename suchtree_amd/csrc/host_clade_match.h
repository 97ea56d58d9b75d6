// host_clade_match.h -- part of suchtree_hip.hip (included after host_unifrac.h).  The device side of st_clade_match
// (kernels_clade_match.h; the checks, the sorted candidates, the windows and the host restatement: clade_match_plan.cpp).
// One work block: pos_b, the rows' ranges and windows, the sorted candidates and two chunks of results.  Per chunk of rows
// one launch of k_clade_match; its 3 int32 per row are copied to one of two pinned buffers (ReadbackRing, host_compare.h)
// and moved to the caller's three arrays while the device works on the next chunk.
#pragma once

// whether rows scan their size windows first: on, or SUCHTREE_AMD_CLADE_MATCH_WINDOW = 0 / 1 for a measurement or a test
// (read at every call); no result depends on it
constexpr bool kCladeMatchWindow = true;

static bool clade_match_window()
{
    const char *e = std::getenv("SUCHTREE_AMD_CLADE_MATCH_WINDOW");
    if (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) return e[0] == '1';
    return kCladeMatchWindow;
}

using CladeMatchRing = ReadbackRing<int32_t, BlockSpan>;

static int clade_match_device(int device, const CladeMatchPlan &P, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi,
                              int32_t *out_distance, int32_t *out_match, int32_t *out_intersection)
{
    const char *what = "clade match";
    if (const int rc = device_index_arg(device); rc != ST_OK) return rc;
    ST_DEVICE(device);
    DevBuf<char> d;      // (declared before the stream's owner)
    CladeMatchRing ring;
    DrainedStream s;
    auto hip_fail = [&](const char *step, hipError_t e) { return fail(ST_ERR_HIP, std::string(what) + step + hipGetErrorString(e)); };
    hipError_t e = s.create();
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    const size_t m = (size_t)P.m, n_a = (size_t)P.n_a, n_b = (size_t)P.n_b, chunk = (size_t)std::min<int64_t>(P.chunk, P.n_a);
    const size_t o_alo = align256(m * 4), o_ahi = o_alo + align256(n_a * 4), o_win = o_ahi + align256(n_a * 4);
    const size_t o_blo = o_win + align256(n_a * 16), o_bhi = o_blo + align256(n_b * 4), o_bidx = o_bhi + align256(n_b * 4);
    const size_t o_out = o_bidx + align256(n_b * 4), out_bytes = align256(chunk * 12), total = o_out + 2 * out_bytes;
    if (const int rc = alloc_work(d, total, ring, chunk * 3, what); rc != ST_OK) return rc;
    char *const base = d;
    e = hipMemcpyAsync(base, pos_b, m * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + o_alo, a_lo, n_a * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + o_ahi, a_hi, n_a * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(base + o_win, P.win.data(), n_a * 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_b > 0) e = hipMemcpyAsync(base + o_blo, P.b_lo.data(), n_b * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_b > 0) e = hipMemcpyAsync(base + o_bhi, P.b_hi.data(), n_b * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_b > 0) e = hipMemcpyAsync(base + o_bidx, P.b_idx.data(), n_b * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(" setup: ", e);
    int *d_out[2] = {reinterpret_cast<int *>(base + o_out), reinterpret_cast<int *>(base + o_out + out_bytes)};
    auto deliver = [&](const int32_t *got, const BlockSpan &rows) {
        for (int64_t r = 0; r < rows.count; r++) {
            out_distance[rows.first + r] = got[3 * r];
            out_match[rows.first + r] = got[3 * r + 1];
            out_intersection[rows.first + r] = got[3 * r + 2];
        }
    };
    const size_t lds = clade_match_lds_bytes(P.m);
    for (int64_t at = 0; at < P.n_a; at += (int64_t)chunk) {
        const int64_t rows = std::min<int64_t>((int64_t)chunk, P.n_a - at);
        e = ring.acquire(deliver);      // (the results of two chunks ago)
        if (e != hipSuccess) return hip_fail(" read-back: ", e);
        int *const out = d_out[ring.next];
        const CladeMatchArgs a{reinterpret_cast<const int *>(base), reinterpret_cast<const int *>(base + o_alo),
                               reinterpret_cast<const int *>(base + o_ahi), reinterpret_cast<const int *>(base + o_win),
                               reinterpret_cast<const int *>(base + o_blo), reinterpret_cast<const int *>(base + o_bhi),
                               reinterpret_cast<const int *>(base + o_bidx), out, P.m, P.n_b, (int)at, (int)rows, P.unrooted ? 1 : 0};
        hipLaunchKernelGGL(k_clade_match, dim3((unsigned)std::min<int64_t>(rows, kCladeMatchBlocks)), dim3(kCladeMatchThreads), lds, s, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = ring.post(out, (size_t)rows * 3, BlockSpan{at, rows}, s);
        if (e != hipSuccess) return hip_fail(" launch: ", e);
    }
    e = ring.drain(deliver, s);
    if (e != hipSuccess) return hip_fail(" read-back: ", e);
    return ST_OK;
}
