// dispersion_plan.cpp -- see dispersion_plan.h.  Argument checks and index arithmetic driven by caller-supplied positions,
// and the restatement of the device reduction operation for operation: no GPU calls.
#include "dispersion_plan.h"
#include "plan_checks.h"

#include <algorithm>
#include <limits>
#include <numeric>

namespace st {

int dispersion_call_args(int32_t n_univ, int64_t permutations, int64_t chunk_tasks, int32_t stream, std::string &err)
{
    if (n_univ < 3 || n_univ > kPermMaxUniverse)
        return fail(ST_ERR_ARG, err, "a universe of " + std::to_string(n_univ) + " positions: 3 to " + std::to_string(kPermMaxUniverse));
    if (permutations < 0) return fail(ST_ERR_ARG, err, "permutations < 0");
    if (chunk_tasks < 0) return fail(ST_ERR_ARG, err, "chunk_tasks < 0");
    if (stream < 0) return fail(ST_ERR_ARG, err, "stream < 0");
    return ST_OK;
}

int matrix_call_args(int32_t n, int64_t permutations, int64_t chunk_tasks, int32_t stream, std::string &err)
{
    if (const int rc = dispersion_call_args(n, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (permutations > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 permutations");
    return ST_OK;
}

// the first cell (row-major) of the square matrix x whose mirror differs, scanned in tiles (the mirror of a row is a
// column); false: x is symmetric
static bool asymmetric(const int32_t *x, int64_t n, int64_t &bad_i, int64_t &bad_j)
{
    constexpr int64_t T = 64;
    bool found = false;
    for (int64_t i0 = 0; i0 < n && !found; i0 += T)
        for (int64_t j0 = 0; j0 <= i0 && !found; j0 += T)
            for (int64_t i = i0; i < std::min(i0 + T, n) && !found; i++)
                for (int64_t j = j0; j < std::min(j0 + T, i); j++)
                    if (x[i * n + j] != x[j * n + i]) {
                        found = true;
                        break;
                    }
    if (!found) return false;
    for (int64_t i = 0; i < n; i++)      // (the error path: which one comes first)
        for (int64_t j = 0; j < n; j++)
            if (x[i * n + j] != x[j * n + i]) {
                bad_i = i;
                bad_j = j;
                return true;
            }
    return false;
}

int symmetric_arg(const char *name, const int32_t *x, int32_t n, std::string &err)
{
    int64_t bi = 0, bj = 0;
    if (!asymmetric(x, n, bi, bj)) return ST_OK;
    const std::string g(name);
    return fail(ST_ERR_ARG, err, g + " is not symmetric: " + g + "[" + std::to_string(bi) + "][" + std::to_string(bj) + "] = " +
                                     std::to_string(x[bi * n + bj]) + ", " + g + "[" + std::to_string(bj) + "][" + std::to_string(bi) + "] = " +
                                     std::to_string(x[bj * n + bi]));
}

void dispersion_cut(int32_t n_univ, int64_t rows, int64_t live, int64_t chunk_tasks, int64_t &perm_block, std::vector<DispersionChunk> &chunks,
                    int64_t &max_chunk_tasks, int64_t table_entries)
{
    dispersion_cut_blocks(rows, live, kDispersionSigmaBytes / (2 * ((int64_t)n_univ + table_entries)), chunk_tasks, perm_block, chunks, max_chunk_tasks);
}

void dispersion_cut_blocks(int64_t rows, int64_t live, int64_t block, int64_t chunk_tasks, int64_t &perm_block, std::vector<DispersionChunk> &chunks,
                           int64_t &max_chunk_tasks, int32_t slice)
{
    block = std::max<int64_t>(1, block);
    int64_t cap = kDispersionChunkTasks;
    if (chunk_tasks > 0) {
        block = std::min(block, chunk_tasks);
        cap = std::min(chunk_tasks, kDispersionMaxChunkTasks);
    }
    perm_block = std::min(block, rows);
    if (live == 0) return;
    for (int64_t p0 = 0; p0 < rows; p0 += perm_block) {
        const int64_t np = std::min(perm_block, rows - p0), tasks = live * dispersion_slices(np, slice);
        for (int64_t t = 0; t < tasks; t += cap) {
            chunks.push_back(DispersionChunk{p0, np, t, std::min(cap, tasks - t)});
            max_chunk_tasks = std::max(max_chunk_tasks, chunks.back().n_tasks);
        }
    }
}

int dispersion_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t permutations,
                    int32_t stream, int64_t chunk_tasks, DispersionPlan &P, std::string &err)
{
    if (const int rc = dispersion_call_args(n_univ, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    const int64_t R = permutations + 1;
    if (n_sets > 0 && R > ((int64_t)1 << 40) / n_sets) return fail(ST_ERR_ARG, err, "more than 2^40 records in one call");
    if (const int rc = position_sets_args(n_univ, set_pos, n_pos, sets, n_sets, err); rc != ST_OK) return rc;
    P = DispersionPlan{};
    P.n_univ = n_univ;
    P.n_sets = n_sets;
    P.rows = R;
    for (int64_t r = 0; r < n_sets; r++)
        if (sets[r + 1] - sets[r] >= 2) P.order.push_back(r);
    dispersion_order(
        P.order, P.class_begin, [&](int64_t r) { return dispersion_class((int)(sets[r + 1] - sets[r])); }, [](int64_t, int64_t) { return false; });
    const int64_t live = (int64_t)P.order.size();
    P.sets.resize((size_t)live);
    for (int64_t c = 0; c < live; c++) {
        const int64_t r = P.order[(size_t)c];
        P.sets[(size_t)c] = DispersionSetDev{(int)sets[r], (int)(sets[r + 1] - sets[r])};
        P.max_count = std::max(P.max_count, P.sets[(size_t)c].count);
    }
    dispersion_cut(n_univ, R, live, chunk_tasks, P.perm_block, P.chunks, P.max_chunk_tasks);
    return ST_OK;
}

void dispersion_butterfly(double *v, int width)
{
    double w[64];
    for (int o = width >> 1; o > 0; o >>= 1) {
        for (int l = 0; l < width; l++) w[l] = v[l] + v[l ^ o];
        std::copy(w, w + width, v);
    }
}

st_dispersion_record dispersion_record(const float *D, int32_t n, const int32_t *q, int32_t k)
{
    if (k < 2) return st_dispersion_record{0.0, 0.0};
    return dispersion_lane_order(k, [&](int32_t i, double &sum, double &near) {
        const float *row = D + (size_t)q[i] * (size_t)n;
        sum = 0.0;
        float m = std::numeric_limits<float>::infinity();
        for (int32_t j = 0; j < k; j++) {
            if (j == i) continue;
            const float v = row[q[j]];
            sum += (double)v;
            m = v < m ? v : m;
        }
        near = (double)m;
    });
}

void dispersion_host(const float *D, const DispersionPlan &P, const int32_t *set_pos, const int64_t *sets, uint64_t seed, int32_t stream,
                     st_dispersion_record *out)
{
    std::vector<int32_t> sigma((size_t)P.n_univ), q((size_t)std::max(P.max_count, 1));
    for (int64_t p = 0; p < P.rows; p++) {
        perm_host(seed, stream, p, 0, P.n_univ, sigma.data());      // (one sigma serves every set)
        for (int64_t r = 0; r < P.n_sets; r++) {
            const int64_t b = sets[r], k = sets[r + 1] - b;
            for (int64_t i = 0; i < k && k >= 2; i++) q[(size_t)i] = sigma[(size_t)set_pos[b + i]];
            out[r * P.rows + p] = dispersion_record(D, P.n_univ, q.data(), (int32_t)k);
        }
    }
}

}  // namespace st
