// group_plan.cpp -- see group_plan.h.  Argument checks, the layout and the restatement of the device sums: no GPU calls.
#include "group_plan.h"

#include <algorithm>

namespace st {

int group_plan(const int32_t *y, int32_t n, const uint8_t *group, int32_t n_groups, int64_t permutations, int32_t stream, int64_t chunk_tasks,
               int32_t slice, const int64_t *out, GroupPlan &P, std::string &err)
{
    if (const int rc = matrix_call_args(n, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (n_groups < 1 || n_groups > kGroupMax) return fail(ST_ERR_ARG, err, std::to_string(n_groups) + " groups: 1 to " + std::to_string(kGroupMax));
    if (!y || !group) return fail(ST_ERR_ARG, err, "y or group is NULL");
    if (!out) return fail(ST_ERR_ARG, err, "out is NULL");
    for (int32_t i = 0; i < n; i++)
        if (group[i] >= n_groups)
            return fail(ST_ERR_ARG, err, "group[" + std::to_string(i) + "] = " + std::to_string((int)group[i]) + " of " + std::to_string(n_groups) + " groups");
    if (slice < 1 || slice > kGroupSliceMax) return fail(ST_ERR_ARG, err, "a slice of " + std::to_string(slice) + " permutations: 1 to " + std::to_string(kGroupSliceMax));
    P = GroupPlan{};
    P.n = n;
    P.n_groups = n_groups;
    P.rows = permutations + 1;
    P.wave = n <= kGroupWaveMax;
    P.items = P.wave ? 1 : ((int64_t)n + 1) / 2;
    P.slice = slice;

    matrix_cut(P, std::min(kDispersionSigmaBytes / (2 * (int64_t)n), kGroupBlockItems / P.items), chunk_tasks, P.wave ? 1 : slice);
    return ST_OK;
}

GroupPart group_row(const int32_t *y_row, const uint8_t *G, int32_t i)
{
    const uint8_t g = G[i];
    int64_t sum = 0;
    for (int32_t j = 0; j < i; j++)
        if (G[j] == g) sum += y_row[j];
    return GroupPart{sum, (int32_t)g, 0};
}

void group_host(const int32_t *y, const uint8_t *group, const GroupPlan &P, uint64_t seed, int32_t stream, int64_t *out)
{
    const int32_t n = P.n;
    std::vector<int32_t> sigma((size_t)n);
    std::vector<uint8_t> G((size_t)n);
    for (int64_t p = 0; p < P.rows; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        for (int32_t j = 0; j < n; j++) G[(size_t)j] = group[sigma[(size_t)j]];
        int64_t *row = out + p * P.n_groups;
        std::fill_n(row, P.n_groups, (int64_t)0);
        for (int64_t i = 1; i < n; i++) {
            const GroupPart part = group_row(y + i * (i - 1) / 2, G.data(), (int32_t)i);
            row[part.g] += part.sum;
        }
    }
}

}  // namespace st
