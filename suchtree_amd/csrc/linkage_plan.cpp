// linkage_plan.cpp -- see linkage_plan.h.  Argument checks and the restatement of the device chain: no GPU calls.
#include "linkage_plan.h"

#include <vector>

namespace st {

int linkage_args(const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, const st_linkage_row *out, std::string &err)
{
    if (n < 2 || n > kLinkageMaxObjects) return fail(ST_ERR_ARG, err, "n = " + std::to_string(n) + " objects: 2 to " + std::to_string(kLinkageMaxObjects));
    if (method != ST_LINKAGE_AVERAGE && method != ST_LINKAGE_SINGLE && method != ST_LINKAGE_COMPLETE)
        return fail(ST_ERR_ARG, err, "method " + std::to_string(method) + ": 0 (average), 1 (single) or 2 (complete)");
    if (!codes || !out) return fail(ST_ERR_ARG, err, "codes or out_rows is NULL");
    const int64_t m = (int64_t)n * (n - 1) / 2;
    for (int64_t k = 0; k < m; k++)
        if (codes[k] < 0) return fail(ST_ERR_ARG, err, "codes[" + std::to_string(k) + "] = " + std::to_string(codes[k]) + " is negative");
    if (weights) {
        int64_t total = 0;
        for (int32_t i = 0; i < n; i++) {
            if (weights[i] < 1) return fail(ST_ERR_ARG, err, "weights[" + std::to_string(i) + "] = " + std::to_string(weights[i]) + ": at least 1");
            total += weights[i];
        }
        if (total > kLinkageMaxWeight) return fail(ST_ERR_ARG, err, "a total weight of " + std::to_string(total) + ": at most " + std::to_string(kLinkageMaxWeight));
    }
    return ST_OK;
}

void linkage_host(const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, st_linkage_row *out, int64_t *rescans)
{
    const size_t N = (size_t)n;
    std::vector<long long> S(N * N, 0), nn_num(N, 0);
    std::vector<int> size(N), id(N), nn_b(N, n);
    for (size_t i = 0; i < N; i++) {
        size[i] = weights ? weights[i] : 1;
        id[i] = (int)i;
    }
    for (size_t i = 1; i < N; i++)
        for (size_t j = 0; j < i; j++) {
            const long long c = codes[i * (i - 1) / 2 + j];
            S[i * N + j] = S[j * N + i] = method == ST_LINKAGE_AVERAGE ? c * size[i] * size[j] : c;
        }
    int64_t scanned = 0;
    auto rescan = [&](size_t k) {
        LinkageCand best = linkage_none();
        const long long *row = &S[k * N];
        for (size_t j = k + 1; j < N; j++) {
            if (!size[j]) continue;
            const LinkageCand c{row[j], linkage_den(method, size[k], size[j]), (int)j, 0};
            if (linkage_before(c, best)) best = c;
        }
        nn_num[k] = best.num;
        nn_b[k] = best.key == kLinkageNone ? n : best.key;
        scanned++;
    };
    for (size_t k = 0; k < N; k++) rescan(k);
    scanned = 0;
    for (int32_t t = 0; t < n - 1; t++) {
        LinkageCand pick = linkage_none();
        for (size_t k = 0; k < N; k++) {
            if (!size[k] || nn_b[k] >= n) continue;
            const LinkageCand c{nn_num[k], linkage_den(method, size[k], size[(size_t)nn_b[k]]), (int)k, nn_b[k]};
            if (linkage_before(c, pick)) pick = c;
        }
        const size_t a = (size_t)pick.key, b = (size_t)pick.aux;
        const long long s_new = (long long)size[a] + size[b];
        out[t] = st_linkage_row{pick.num, pick.den, id[a] < id[b] ? id[a] : id[b], id[a] < id[b] ? id[b] : id[a], s_new};
        long long *Sa = &S[a * N];
        const long long *Sb = &S[b * N];
        for (size_t k = 0; k < N; k++) {
            if (!size[k] || k == a || k == b) continue;
            Sa[k] = S[k * N + a] = linkage_merge(method, Sa[k], Sb[k]);
        }
        size[a] = (int)s_new;
        size[b] = 0;
        id[a] = n + t;
        for (size_t k = 0; k < b; k++) {
            if (!size[k] || k == a) continue;
            const bool lost = nn_b[k] == (int)b || (k < a && nn_b[k] == (int)a);
            if (lost) {
                rescan(k);
            } else if (k < a) {
                const LinkageCand now{Sa[k], linkage_den(method, size[k], s_new), (int)a, 0};
                const LinkageCand cur{nn_num[k], linkage_den(method, size[k], size[(size_t)nn_b[k]]), nn_b[k], 0};
                if (linkage_before(now, cur)) {
                    nn_num[k] = now.num;
                    nn_b[k] = (int)a;
                }
            }
        }
        rescan(a);
    }
    if (rescans) *rescans = scanned;
}

}  // namespace st
