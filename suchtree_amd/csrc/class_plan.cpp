// class_plan.cpp -- see class_plan.h.  Argument checks, the layout and the restatement of the device sums: no GPU calls.
#include "class_plan.h"

#include <algorithm>

namespace st {

int class_plan(const int32_t *y, const uint8_t *cls, int32_t n, int32_t n_classes, int64_t permutations, int32_t stream, int64_t chunk_tasks,
               int32_t slice, const int64_t *out, ClassPlan &P, std::string &err)
{
    if (const int rc = matrix_call_args(n, permutations, chunk_tasks, stream, err); rc != ST_OK) return rc;
    if (n_classes < 1 || n_classes > kClassMax) return fail(ST_ERR_ARG, err, std::to_string(n_classes) + " classes: 1 to " + std::to_string(kClassMax));
    if (!y || !cls) return fail(ST_ERR_ARG, err, "y or cls is NULL");
    if (!out) return fail(ST_ERR_ARG, err, "out is NULL");
    const int64_t m = (int64_t)n * (n - 1) / 2;
    for (int64_t k = 0; k < m; k++)
        if (cls[k] >= n_classes && cls[k] != kClassNone)
            return fail(ST_ERR_ARG, err, "cls[" + std::to_string(k) + "] = " + std::to_string((int)cls[k]) + " of " + std::to_string(n_classes) + " classes");
    if (slice < 1 || slice > kClassSliceMax) return fail(ST_ERR_ARG, err, "a slice of " + std::to_string(slice) + " permutations: 1 to " + std::to_string(kClassSliceMax));
    P = ClassPlan{};
    P.n = n;
    P.n_classes = n_classes;
    P.rows = permutations + 1;
    P.wave = n <= kClassWaveMax;
    P.items = P.wave ? 1 : ((int64_t)n + 1) / 2;
    P.slice = slice;

    matrix_cut(P, std::min(kDispersionSigmaBytes / (2 * (int64_t)n), kClassPartBytes / (8 * (int64_t)n_classes * P.items)), chunk_tasks, P.wave ? 1 : slice);
    return ST_OK;
}

void class_row(const int32_t *y_row, const uint8_t *cls, const int32_t *sigma, int32_t i, int64_t *acc)
{
    const int32_t si = sigma[i];
    for (int32_t j = 0; j < i; j++) {
        const uint8_t c = cls[class_pair(si, sigma[j])];
        if (c != kClassNone) acc[c] += y_row[j];
    }
}

void class_host(const int32_t *y, const uint8_t *cls, const ClassPlan &P, uint64_t seed, int32_t stream, int64_t *out)
{
    const int32_t n = P.n;
    std::vector<int32_t> sigma((size_t)n);
    for (int64_t p = 0; p < P.rows; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        int64_t *row = out + p * P.n_classes;
        std::fill_n(row, P.n_classes, (int64_t)0);
        for (int64_t i = 1; i < n; i++) class_row(y + i * (i - 1) / 2, cls, sigma.data(), (int32_t)i, row);
    }
}

}  // namespace st
