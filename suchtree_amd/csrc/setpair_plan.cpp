// setpair_plan.cpp -- see setpair_plan.h.  Argument checks and index arithmetic driven by caller-supplied positions, and
// the restatement of the device reduction operation for operation: no GPU calls.
#include "setpair_plan.h"
#include "plan_checks.h"

#include <algorithm>
#include <limits>

namespace st {

int setpair_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t begin, int64_t count,
                 int32_t exclude_shared, int64_t permutations, int32_t stream, int64_t chunk_tasks, SetpairPlan &P, std::string &err)
{
    if (const int rc = dispersion_call_args(n_univ, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (const int rc = position_sets_args(n_univ, set_pos, n_pos, sets, n_sets, err); rc != ST_OK) return rc;
    if (begin < 0 || count < 0) return fail(ST_ERR_ARG, err, "a negative triangle range");
    const int64_t total = n_sets > ((int64_t)1 << 31) ? std::numeric_limits<int64_t>::max() : n_sets * (n_sets - 1) / 2;
    if (const int rc = triangle_range_args(total, begin, count, err); rc != ST_OK) return rc;
    if (count > kSetpairMaxPairs) return fail(ST_ERR_ARG, err, "more than 2^31 pairs in one call");
    const int64_t R = permutations + 1;
    if (count > 0 && R > ((int64_t)1 << 39) / count) return fail(ST_ERR_ARG, err, "more than 2^40 records in one call");
    P = SetpairPlan{};
    P.n_univ = n_univ;
    P.n_sets = n_sets;
    P.rows = R;
    P.begin = begin;
    P.count = count;
    P.exclude = exclude_shared != 0;
    auto size = [&](int64_t r) { return (int)(sets[r + 1] - sets[r]); };
    std::vector<SetpairTaskDev> all((size_t)(2 * count));      // by direction u
    int64_t i = 0, j = 0;
    if (count > 0) unifrac_pair(begin, i, j);
    for (int64_t u = 0; u < 2 * count; u += 2) {
        all[(size_t)u] = SetpairTaskDev{(int)sets[i], size(i), (int)sets[j], size(j)};
        all[(size_t)u + 1] = SetpairTaskDev{(int)sets[j], size(j), (int)sets[i], size(i)};
        if (++j == i) {
            i++;
            j = 0;
        }
    }
    for (int64_t u = 0; u < 2 * count; u++)
        if (all[(size_t)u].r_count >= 1 && all[(size_t)u].c_count >= 1) P.order.push_back(u);
    dispersion_order(
        P.order, P.class_begin, [&](int64_t u) { return dispersion_class(all[(size_t)u].r_count); },
        [&](int64_t a, int64_t b) { return all[(size_t)a].c_count < all[(size_t)b].c_count; });
    const int64_t live = (int64_t)P.order.size();
    P.tasks.resize((size_t)live);
    for (int64_t c = 0; c < live; c++) {
        P.tasks[(size_t)c] = all[(size_t)P.order[(size_t)c]];
        if (c >= P.class_begin[kDispersionClasses - 1]) P.max_walk = std::max(P.max_walk, P.tasks[(size_t)c].c_count);
    }
    dispersion_cut(n_univ, R, live, chunk_tasks, P.perm_block, P.chunks, P.max_chunk_tasks);
    return ST_OK;
}

st_dispersion_record setpair_record(const float *D, int32_t n, const int32_t *qr, const int32_t *sr, int32_t kr, const int32_t *qc,
                                    const int32_t *sc, int32_t kc, bool exclude)
{
    if (kr < 1) return st_dispersion_record{0.0, 0.0};
    return dispersion_lane_order(kr, [&](int32_t i, double &sum, double &near) {
        const float *row = D + (size_t)qr[i] * (size_t)n;
        sum = 0.0;
        float m = std::numeric_limits<float>::infinity();
        for (int32_t j = 0; j < kc; j++) {
            if (exclude && sc[j] == sr[i]) continue;
            const float v = row[qc[j]];
            sum += (double)v;
            m = v < m ? v : m;
        }
        // no included entry: by the sets alone, never by the value of m
        const bool none = kc == 0 || (exclude && kc == 1 && sc[0] == sr[i]);
        near = none ? 0.0 : (double)m;
    });
}

void setpair_host(const float *D, const SetpairPlan &P, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, uint64_t seed, int32_t stream,
                  st_dispersion_record *out)
{
    std::vector<int32_t> sigma((size_t)P.n_univ), q((size_t)std::max<int64_t>(n_pos, 1));
    for (int64_t p = 0; p < P.rows && P.count > 0; p++) {
        perm_host(seed, stream, p, 0, P.n_univ, sigma.data());      // (one sigma serves every set)
        for (int64_t x = 0; x < n_pos; x++) q[(size_t)x] = sigma[(size_t)set_pos[x]];
        int64_t i, j;
        unifrac_pair(P.begin, i, j);
        for (int64_t k = 0; k < P.count; k++) {
            const int64_t bi = sets[i], ki = sets[i + 1] - bi, bj = sets[j], kj = sets[j + 1] - bj;
            out[(2 * k) * P.rows + p] =
                setpair_record(D, P.n_univ, q.data() + bi, set_pos + bi, (int32_t)ki, q.data() + bj, set_pos + bj, (int32_t)kj, P.exclude != 0);
            out[(2 * k + 1) * P.rows + p] =
                setpair_record(D, P.n_univ, q.data() + bj, set_pos + bj, (int32_t)kj, q.data() + bi, set_pos + bi, (int32_t)ki, P.exclude != 0);
            if (++j == i) {
                i++;
                j = 0;
            }
        }
    }
}

}  // namespace st
