// rf_plan.cpp -- see rf_plan.h.  The argument checks, the tables a call uploads and the restatement of the kernel's
// method: no GPU calls.
#include "rf_plan.h"

#include <algorithm>
#include <numeric>

namespace st {

// row r of a table of permutations of 0 .. m - 1
static int permutation_row(const char *name, const int32_t *row, int64_t r, int32_t m, std::vector<char> &seen, std::string &err)
{
    std::fill(seen.begin(), seen.end(), 0);
    for (int32_t k = 0; k < m; k++) {
        const int32_t v = row[k];
        if (v < 0 || v >= m || seen[(size_t)v])
            return fail(ST_ERR_ARG, err, std::string(name) + "[" + std::to_string(r) + "][" + std::to_string(k) + "] = " + std::to_string(v) +
                                             ": every row of " + name + " must be a permutation of 0 .. m - 1");
        seen[(size_t)v] = 1;
    }
    return ST_OK;
}

int rf_plan(int32_t m, int32_t n_trees, const int32_t *where, const int64_t *clade_offsets, const int32_t *lo, const int32_t *hi, bool unrooted,
            const int32_t *align, int32_t n_align, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int64_t n_tasks,
            int64_t begin, int64_t chunk_tasks, const int32_t *out_shared, RfPlan &P, std::string &err)
{
    P = RfPlan{};
    if (m < kRfMinLeaves || m > kRfMaxLeaves)
        return fail(ST_ERR_ARG, err, "a list of " + std::to_string(m) + " leaves: " + std::to_string(kRfMinLeaves) + " to " + std::to_string(kRfMaxLeaves));
    if (n_trees < 0 || n_align < 0 || n_tasks < 0) return fail(ST_ERR_ARG, err, "negative size");
    if (begin < 0) return fail(ST_ERR_ARG, err, "begin < 0");
    if (chunk_tasks < 0) return fail(ST_ERR_ARG, err, "chunk_tasks < 0");
    if (n_trees > 0 && (!where || !clade_offsets)) return fail(ST_ERR_ARG, err, "where or clade_offsets is NULL");
    if (n_align > 0 && !align) return fail(ST_ERR_ARG, err, "align is NULL");
    if (n_trees == 0 && n_tasks > 0) return fail(ST_ERR_ARG, err, "tasks without trees");
    if (n_trees > 0 && clade_offsets[0] != 0) return fail(ST_ERR_ARG, err, "clade_offsets[0] = " + std::to_string(clade_offsets[0]) + ": the offsets start at 0");
    for (int32_t t = 0; t < n_trees; t++)
        if (clade_offsets[t + 1] < clade_offsets[t] || clade_offsets[t + 1] > INT32_MAX)
            return fail(ST_ERR_ARG, err, "clade_offsets[" + std::to_string(t + 1) + "] = " + std::to_string(clade_offsets[t + 1]) +
                                             ": the offsets must not decrease and stay below 2^31");
    const int64_t n_clades = n_trees > 0 ? clade_offsets[n_trees] : 0;
    if (n_clades > 0 && (!lo || !hi)) return fail(ST_ERR_ARG, err, "lo or hi is NULL");
    std::vector<char> seen((size_t)m);
    for (int32_t t = 0; t < n_trees; t++)
        if (const int rc = permutation_row("where", where + (size_t)t * (size_t)m, t, m, seen, err); rc != ST_OK) return rc;
    for (int32_t t = 0; t < n_trees; t++)
        for (int64_t c = clade_offsets[t]; c < clade_offsets[t + 1]; c++)
            if (lo[c] < 0 || hi[c] <= lo[c] || hi[c] > m)
                return fail(ST_ERR_ARG, err, "tree " + std::to_string(t) + ", range " + std::to_string(c - clade_offsets[t]) + ": [" + std::to_string(lo[c]) +
                                                 ", " + std::to_string(hi[c]) + ") of " + std::to_string(m) + " positions");
    for (int32_t r = 0; r < n_align; r++)
        if (const int rc = permutation_row("align", align + (size_t)r * (size_t)m, r, m, seen, err); rc != ST_OK) return rc;
    const bool triangle = !task_i && !task_j;
    if (triangle) {
        if (task_p) return fail(ST_ERR_ARG, err, "task_p without task_i and task_j");
        const int64_t total = (int64_t)n_trees * (n_trees - 1) / 2;
        if (const int rc = triangle_range_args(total > 0 ? total : 0, begin, n_tasks, err); rc != ST_OK) return rc;
    } else {
        if (!task_i || !task_j) return fail(ST_ERR_ARG, err, "task_i or task_j is NULL");
        if (begin != 0) return fail(ST_ERR_ARG, err, "begin = " + std::to_string(begin) + " with explicit tasks");
        for (int64_t t = 0; t < n_tasks; t++) {
            if (task_i[t] < 0 || task_i[t] >= n_trees || task_j[t] < 0 || task_j[t] >= n_trees)
                return fail(ST_ERR_BOUNDS, err, "task " + std::to_string(t) + ": trees (" + std::to_string(task_i[t]) + ", " + std::to_string(task_j[t]) +
                                                    ") of " + std::to_string(n_trees));
            if (task_p && (task_p[t] < -1 || task_p[t] >= n_align))
                return fail(ST_ERR_BOUNDS, err, "task " + std::to_string(t) + ": alignment " + std::to_string(task_p[t]) + " of " + std::to_string(n_align));
        }
    }
    if (n_tasks > 0 && !out_shared) return fail(ST_ERR_ARG, err, "out_shared is NULL");
    P.m = m;
    P.n_trees = n_trees;
    P.n_align = n_align;
    P.unrooted = unrooted;
    P.triangle = triangle;
    P.n_tasks = n_tasks;
    P.begin = begin;
    P.chunk = std::max<int64_t>(1, std::min({chunk_tasks > 0 ? chunk_tasks : kRfChunkTasks, n_tasks, kRfChunkTasksMax}));
    P.n_clades = n_clades;
    P.where.resize((size_t)n_trees * (size_t)m);
    for (size_t k = 0; k < P.where.size(); k++) P.where[k] = (uint16_t)where[k];
    P.align.resize((size_t)n_align * (size_t)m);
    for (size_t k = 0; k < P.align.size(); k++) P.align[k] = (uint16_t)align[k];
    P.off.resize((size_t)n_trees + 1, 0);
    P.range.resize((size_t)n_clades);
    P.key.resize((size_t)n_clades);
    P.idx.resize((size_t)n_clades);
    std::vector<int32_t> by;
    for (int32_t t = 0; t < n_trees; t++) {
        const int64_t c0 = clade_offsets[t], n = clade_offsets[t + 1] - c0;
        P.off[(size_t)t + 1] = (int32_t)(c0 + n);
        by.resize((size_t)n);
        std::iota(by.begin(), by.end(), 0);
        auto canonical = [&](int32_t r) { return rf_canonical(lo[c0 + r], hi[c0 + r], m, unrooted); };
        std::stable_sort(by.begin(), by.end(), [&](int32_t x, int32_t y) { return canonical(x) < canonical(y); });
        for (int64_t r = 0; r < n; r++) {
            P.range[(size_t)(c0 + r)] = rf_key(lo[c0 + r], hi[c0 + r]);
            P.key[(size_t)(c0 + r)] = canonical(by[(size_t)r]);
            P.idx[(size_t)(c0 + r)] = by[(size_t)r];
        }
    }
    return ST_OK;
}

void rf_host(const RfPlan &P, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int32_t *out_shared, int64_t *out_count)
{
    const int m = P.m, nb = rf_blocks(m), stride = rf_stride(nb), levels = rf_levels(nb);
    const size_t M = (size_t)m;
    std::vector<uint16_t> q(M), tmin((size_t)levels * (size_t)stride, 0), tmax(tmin);
    if (out_count) std::fill(out_count, out_count + P.n_clades, (int64_t)0);
    for (int64_t t = 0; t < P.n_tasks; t++) {
        int32_t i, j, p;
        rf_task(P, task_i, task_j, task_p, t, i, j, p);
        const uint16_t *wi = &P.where[(size_t)i * M], *wj = &P.where[(size_t)j * M], *al = p >= 0 ? &P.align[(size_t)p * M] : nullptr;
        int noted = 0;
        for (int k = 0; k < m; k++) {
            const int y = wj[al ? al[k] : k];
            q[(size_t)y] = wi[k];
            if (wi[k] == 0) noted = y;
        }
        for (int b = 0; b < nb; b++) {
            const int end = std::min(m, b * 64 + 64);
            tmin[(size_t)b] = *std::min_element(q.begin() + b * 64, q.begin() + end);
            tmax[(size_t)b] = *std::max_element(q.begin() + b * 64, q.begin() + end);
        }
        for (int l = 1; l < levels; l++)
            for (int b = 0; b + (1 << l) <= nb; b++) {
                const size_t to = (size_t)(l * stride + b), x = (size_t)((l - 1) * stride + b), y = x + ((size_t)1 << (l - 1));
                tmin[to] = std::min(tmin[x], tmin[y]);
                tmax[to] = std::max(tmax[x], tmax[y]);
            }
        const int32_t c0 = P.off[(size_t)j], nj = P.off[(size_t)j + 1] - c0, k0 = P.off[(size_t)i], ni = P.off[(size_t)i + 1] - k0;
        int32_t shared = 0;
        for (int32_t c = 0; c < nj; c++) {
            const uint32_t r = P.range[(size_t)(c0 + c)];
            const uint32_t key = rf_clade_key(q.data(), tmin.data(), tmax.data(), stride, m, (int)(r >> 16), (int)(r & 0xFFFFu), P.unrooted, noted);
            if (key == kRfNoKey) continue;
            const int at = rf_find(P.key.data() + k0, ni, key);
            if (at < 0) continue;
            shared++;
            if (out_count) {
                out_count[c0 + c]++;
                out_count[k0 + P.idx[(size_t)(k0 + at)]]++;
            }
        }
        out_shared[t] = shared;
    }
}

}  // namespace st
