// unifrac_plan.cpp -- see unifrac_plan.h.  Argument checks, the quantiser, the chunk cut and the restatement of the device
// reduction: no GPU calls.
#include "unifrac_plan.h"
#include "plan_checks.h"

#include <algorithm>
#include <cmath>

namespace st {

static int universe_arg(int32_t n, std::string &err)
{
    if (n < 1 || n > kUnifracMaxUniverse)
        return fail(ST_ERR_ARG, err, "a universe of " + std::to_string(n) + " positions: 1 to " + std::to_string(kUnifracMaxUniverse));
    return ST_OK;
}

int unifrac_plan(int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count,
                 int64_t chunk_pairs, bool want_pd, bool want_union, UnifracPlan &P, std::string &err)
{
    if (const int rc = universe_arg(n, err); rc != ST_OK) return rc;
    if (chunk_pairs < 0) return fail(ST_ERR_ARG, err, "chunk_pairs < 0");
    if (k_begin < 0 || k_count < 0) return fail(ST_ERR_ARG, err, "a negative triangle range");
    if (n_sets > ((int64_t)1 << 30)) return fail(ST_ERR_ARG, err, "more than 2^30 sets");
    if (const int rc = position_sets_args(n, set_pos, n_pos, sets, n_sets, err); rc != ST_OK) return rc;
    if (const int rc = triangle_range_args(n_sets > 0 ? n_sets * (n_sets - 1) / 2 : 0, k_begin, k_count, err); rc != ST_OK) return rc;
    P = UnifracPlan{};
    P.n = n;
    P.m = (int64_t)n - 1;
    P.levels = unifrac_levels(P.m);
    P.n_sets = n_sets;
    P.k_begin = k_begin;
    P.k_count = k_count;
    const int64_t cap = chunk_pairs > 0 ? std::min(chunk_pairs, kUnifracMaxChunkPairs) : kUnifracChunkPairs;
    auto cut = [&](int kind, int64_t begin, int64_t count) {
        for (int64_t at = 0; at < count; at += cap) {
            P.chunks.push_back(UnifracChunk{kind, begin + at, std::min(cap, count - at), at});
            P.max_chunk = std::max(P.max_chunk, P.chunks.back().count);
        }
    };
    if (want_pd) cut(kUnifracPD, 0, n_sets);
    if (want_union) cut(kUnifracPairs, k_begin, k_count);
    return ST_OK;
}

int unifrac_shift_arg(int32_t shift, std::string &err)
{
    if (shift < -1 || shift > kUnifracMaxShift) return fail(ST_ERR_ARG, err, "shift must be -1 (automatic) or 0 to " + std::to_string(kUnifracMaxShift));
    return ST_OK;
}

int unifrac_quantise(const float *d, const float *h, int32_t n, int32_t shift, int64_t *d_q, int64_t *h_q, int32_t *shift_used, std::string &err)
{
    if (const int rc = universe_arg(n, err); rc != ST_OK) return rc;
    if (!d || (n > 1 && !h)) return fail(ST_ERR_ARG, err, "d or h is NULL");
    if (const int rc = unifrac_shift_arg(shift, err); rc != ST_OK) return rc;
    float top = 0.0f;
    for (int32_t k = 0; k < 2 * n - 1; k++) {
        const float v = k < n ? d[k] : h[k - n];
        if (!std::isfinite(v)) return fail(ST_ERR_ARG, err, std::string(k < n ? "d[" : "h[") + std::to_string(k < n ? k : k - n) + "] is not finite");
        top = std::max(top, std::fabs(v));
    }
    int s = shift;
    if (shift < 0) s = top == 0.0f ? 0 : 39 - std::ilogb(top);      // (top 2^(39 - s) is an integer in [2^39, 2^40): 24 bits, scaled up)
    if (std::fabs(std::ldexp((double)top, s)) >= (double)kUnifracQLimit)
        return fail(ST_ERR_ARG, err, "shift " + std::to_string(s) + " puts the largest depth, " + std::to_string(top) + ", at 2^40 or more");
    for (int32_t k = 0; k < n; k++)
        if (d_q) d_q[k] = std::llrint(std::ldexp((double)d[k], s));
    for (int32_t k = 0; k + 1 < n; k++)
        if (h_q) h_q[k] = std::llrint(std::ldexp((double)h[k], s));
    if (shift_used) *shift_used = s;
    return ST_OK;
}

int unifrac_depth_args(const int64_t *d_q, const int64_t *h_q, int32_t n, std::string &err)
{
    if (const int rc = universe_arg(n, err); rc != ST_OK) return rc;
    if (!d_q || (n > 1 && !h_q)) return fail(ST_ERR_ARG, err, "d_q or h_q is NULL");
    for (int32_t k = 0; k < 2 * n - 1; k++) {
        const int64_t v = k < n ? d_q[k] : h_q[k - n];
        if (v <= -kUnifracQLimit || v >= kUnifracQLimit)
            return fail(ST_ERR_ARG, err, std::string(k < n ? "d_q[" : "h_q[") + std::to_string(k < n ? k : k - n) + "] is 2^40 or more in size");
    }
    return ST_OK;
}

void unifrac_table(const int64_t *h_q, int64_t m, int levels, int64_t *M)
{
    std::copy(h_q, h_q + (levels > 0 ? m : 0), M);
    for (int l = 1; l < levels; l++) {
        const int64_t half = (int64_t)1 << (l - 1), *below = M + (int64_t)(l - 1) * m;
        int64_t *row = M + (int64_t)l * m;
        for (int64_t k = 0; k + 2 * half <= m; k++) row[k] = std::min(below[k], below[k + half]);
    }
}

int64_t unifrac_union(const int64_t *d_q, const int64_t *M, int64_t m, const int32_t *A, int64_t na, const int32_t *B, int64_t nb)
{
    int64_t sum = 0, a = 0, b = 0;
    int32_t prev = -1;
    while (a < na || b < nb) {
        const int32_t x = a < na ? A[a] : INT32_MAX, y = b < nb ? B[b] : INT32_MAX, c = std::min(x, y);
        a += x == c;
        b += y == c;
        sum += d_q[c];
        if (prev >= 0) sum -= unifrac_rmq(M, m, prev, c);
        prev = c;
    }
    return sum;
}

// d_q[x] - min h_q[x .. next - 1], or d_q[x] for the union's last element (next = INT32_MAX)
static int64_t successor_term(const int64_t *d_q, const int64_t *M, int64_t m, int32_t x, int32_t next)
{
    return next == INT32_MAX ? d_q[x] : d_q[x] - unifrac_rmq(M, m, x, next);
}

int64_t unifrac_union_successor(const int64_t *d_q, const int64_t *M, int64_t m, const int32_t *A, int64_t na, const int32_t *B, int64_t nb)
{
    int64_t sum = 0;
    for (int64_t e = 0; e < na; e++) {
        const int32_t x = A[e], in_a = e + 1 < na ? A[e + 1] : INT32_MAX;
        const int32_t *up = std::upper_bound(B, B + nb, x);
        sum += successor_term(d_q, M, m, x, std::min(in_a, up < B + nb ? *up : INT32_MAX));
    }
    for (int64_t e = 0; e < nb; e++) {
        const int32_t y = B[e], in_b = e + 1 < nb ? B[e + 1] : INT32_MAX;
        const int32_t *lo = std::lower_bound(A, A + na, y);
        if (lo < A + na && *lo == y) continue;      // (counted with A)
        sum += successor_term(d_q, M, m, y, std::min(in_b, lo < A + na ? *lo : INT32_MAX));
    }
    return sum;
}

void unifrac_host(const int64_t *d_q, const int64_t *h_q, const UnifracPlan &P, const int32_t *set_pos, const int64_t *sets, int64_t *out_pd,
                  int64_t *out_union)
{
    std::vector<int64_t> M((size_t)(P.levels * P.m));
    unifrac_table(h_q, P.m, P.levels, M.data());
    for (const UnifracChunk &c : P.chunks) {
        int64_t *out = (c.kind == kUnifracPD ? out_pd : out_union) + c.out_at;
        for (int64_t t = 0; t < c.count; t++) {
            int64_t i = c.begin + t, j = i;
            if (c.kind == kUnifracPairs) unifrac_pair(c.begin + t, i, j);
            out[t] = unifrac_union(d_q, M.data(), P.m, set_pos + sets[j], sets[j + 1] - sets[j], set_pos + sets[i], sets[i + 1] - sets[i]);
        }
    }
}

}  // namespace st
