// unifrac_null_plan.cpp -- see unifrac_null_plan.h.  Argument checks, the layout and the plain restatement that the kernels
// are held to: no GPU calls.
#include "unifrac_null_plan.h"
#include "plan_checks.h"

#include <algorithm>

namespace st {

int unifrac_null_plan(int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t k_begin, int64_t k_count,
                      int64_t permutations, int32_t stream, int64_t chunk_tasks, bool want_pd, bool want_union, UnifracNullPlan &P,
                      std::string &err)
{
    if (const int rc = dispersion_call_args(n, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (const int rc = position_sets_args(n, set_pos, n_pos, sets, n_sets, err); rc != ST_OK) return rc;
    if (k_begin < 0 || k_count < 0) return fail(ST_ERR_ARG, err, "a negative triangle range");
    if (n_sets > ((int64_t)1 << 30)) return fail(ST_ERR_ARG, err, "more than 2^30 sets");
    if (const int rc = triangle_range_args(n_sets > 0 ? n_sets * (n_sets - 1) / 2 : 0, k_begin, k_count, err); rc != ST_OK) return rc;
    const int64_t R = permutations + 1, most = std::max(n_sets, k_count);
    if (most > 0 && R > ((int64_t)1 << 40) / most) return fail(ST_ERR_ARG, err, "more than 2^40 values in one output array");
    P = UnifracNullPlan{};
    P.n = n;
    P.m = (int64_t)n - 1;
    P.levels = unifrac_levels(P.m);
    P.n_sets = n_sets;
    P.k_begin = k_begin;
    P.k_count = k_count;
    P.rows = R;
    P.want_pd = want_pd;
    P.want_union = want_union && k_count > 0;
    P.n_tab = P.want_union ? n_pos : 0;
    P.items = P.want_union ? n_sets + k_count : P.want_pd ? n_sets : 0;
    dispersion_cut(n, R, P.items, chunk_tasks, P.perm_block, P.chunks, P.max_chunk_tasks, P.n_tab);
    return ST_OK;
}

void unifrac_null_host(const int64_t *d_q, const int64_t *h_q, const UnifracNullPlan &P, const int32_t *set_pos, int64_t n_pos,
                       const int64_t *sets, uint64_t seed, int32_t stream, int64_t *out_pd, int64_t *out_union)
{
    if (P.items == 0) return;
    std::vector<int64_t> M((size_t)(P.levels * P.m));
    unifrac_table(h_q, P.m, P.levels, M.data());
    std::vector<int32_t> sigma((size_t)P.n);
    std::vector<std::vector<int32_t>> R((size_t)P.n_sets);
    (void)n_pos;
    for (int64_t p = 0; p < P.rows; p++) {
        perm_host(seed, stream, p, 0, P.n, sigma.data());      // (one sigma serves every set)
        for (int64_t r = 0; r < P.n_sets; r++) {
            std::vector<int32_t> &q = R[(size_t)r];
            q.clear();
            for (int64_t x = sets[r]; x < sets[r + 1]; x++) q.push_back(sigma[(size_t)set_pos[x]]);
            std::sort(q.begin(), q.end());
            if (P.want_pd) out_pd[r * P.rows + p] = unifrac_union(d_q, M.data(), P.m, q.data(), (int64_t)q.size(), q.data(), (int64_t)q.size());
        }
        for (int64_t k = 0; k < P.k_count && P.want_union; k++) {
            int64_t i, j;
            unifrac_pair(P.k_begin + k, i, j);
            const std::vector<int32_t> &A = R[(size_t)j], &B = R[(size_t)i];
            out_union[k * P.rows + p] = unifrac_union(d_q, M.data(), P.m, A.data(), (int64_t)A.size(), B.data(), (int64_t)B.size());
        }
    }
}

void unifrac_null_scatter(const UnifracNullPlan &P, const DispersionChunk &c, const int64_t *results, int64_t *out_pd, int64_t *out_union)
{
    for (int64_t j = 0; j < c.n_tasks; j++) {
        int64_t s, p;
        dispersion_task_of(c, j, s, p);
        if (s < P.n_sets) {
            if (P.want_pd) out_pd[s * P.rows + p] = results[j];
        } else {
            out_union[(s - P.n_sets) * P.rows + p] = results[j];
        }
    }
}

}  // namespace st
