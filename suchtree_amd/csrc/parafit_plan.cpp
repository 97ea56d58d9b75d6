// parafit_plan.cpp -- see parafit_plan.h.  Argument checks, the layout and the restatement of the device records: no GPU
// calls.
#include "parafit_plan.h"

#include <algorithm>

namespace st {

int parafit_plan(const int32_t *g_f, int32_t n_f, const int32_t *g_s, int32_t n_s, const int32_t *link_f, const int32_t *link_s, int32_t n_links,
                 const int32_t *stream_f, int64_t permutations, int64_t chunk_tasks, const st_parafit_sum *total, const st_parafit_sum *link_obs,
                 const int64_t *link_n_ge, ParafitPlan &P, std::string &err)
{
    const std::string range = ": 3 to " + std::to_string(kPermMaxUniverse);
    if (n_f < 3 || n_f > kPermMaxUniverse) return fail(ST_ERR_ARG, err, "n_f = " + std::to_string(n_f) + range);
    if (n_s < 3 || n_s > kPermMaxUniverse) return fail(ST_ERR_ARG, err, "n_s = " + std::to_string(n_s) + range);
    if (n_links < 3 || n_links > kPermMaxUniverse) return fail(ST_ERR_ARG, err, "n_links = " + std::to_string(n_links) + range);
    if (permutations < 0 || chunk_tasks < 0) return fail(ST_ERR_ARG, err, "permutations or chunk_tasks < 0");
    if (permutations > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 permutations");
    if (!g_f || !g_s || !link_f || !link_s || !stream_f) return fail(ST_ERR_ARG, err, "g_f, g_s, link_f, link_s or stream_f is NULL");
    if (!total || !link_obs || !link_n_ge) return fail(ST_ERR_ARG, err, "total, link_obs or link_n_ge is NULL");
    for (int32_t l = 0; l < n_links; l++) {
        const std::string at = "link " + std::to_string(l) + " (" + std::to_string(link_f[l]) + ", " + std::to_string(link_s[l]) + ")";
        if (link_f[l] < 0 || link_f[l] >= n_f) return fail(ST_ERR_ARG, err, at + ": the F position is outside the universe of " + std::to_string(n_f));
        if (link_s[l] < 0 || link_s[l] >= n_s) return fail(ST_ERR_ARG, err, at + ": the S position is outside the universe of " + std::to_string(n_s));
        if (l > 0 && (link_f[l] < link_f[l - 1] || (link_f[l] == link_f[l - 1] && link_s[l] <= link_s[l - 1])))
            return fail(ST_ERR_ARG, err, at + ": the links must be strictly increasing in (f, s) order");
    }
    for (int32_t i = 0; i < n_f; i++)
        if (stream_f[i] < 0) return fail(ST_ERR_ARG, err, "stream_f[" + std::to_string(i) + "] < 0");
    if (const int rc = symmetric_arg("g_f", g_f, n_f, err); rc != ST_OK) return rc;
    if (const int rc = symmetric_arg("g_s", g_s, n_s, err); rc != ST_OK) return rc;

    P = ParafitPlan{};
    P.n_f = n_f;
    P.n_s = n_s;
    P.n_links = n_links;
    P.rows = permutations + 1;
    P.wave = n_links <= kParafitWaveMax && n_s <= kParafitWaveMax;
    P.items = P.wave ? 1 : n_links;
    for (int32_t l = 0; l < n_links; l++) {
        if (l == 0 || link_f[l] != link_f[l - 1]) P.groups.push_back(ParafitGroup{link_f[l], stream_f[link_f[l]], l, 0});
        P.groups.back().count++;
    }

    const int64_t L = n_links;
    matrix_cut(P, std::min(kDispersionSigmaBytes / (2 * L), kParafitBlockTasks / L), chunk_tasks);
    return ST_OK;
}

void parafit_relabel(const ParafitPlan &P, const int32_t *link_s, uint64_t seed, int64_t p, int32_t *r)
{
    std::vector<int32_t> sigma((size_t)P.n_s);
    for (const ParafitGroup &g : P.groups) {
        perm_host(seed, g.stream, p, 0, P.n_s, sigma.data());
        for (int32_t l = g.begin; l < g.begin + g.count; l++) r[l] = sigma[(size_t)link_s[l]];
    }
}

void parafit_records(const int32_t *g_f, const int32_t *g_s, const ParafitPlan &P, const int32_t *link_f, const int32_t *r, ParafitRecord *rec, i128 &total)
{
    const int64_t L = P.n_links;
    total = 0;
    for (int64_t l = 0; l < L; l++) {
        const int32_t *fr = g_f + (int64_t)link_f[l] * P.n_f, *sr = g_s + (int64_t)r[l] * P.n_s;
        i128 row = 0;
        for (int64_t k = 0; k < L; k++) row += (i128)((int64_t)fr[link_f[k]] * (int64_t)sr[r[k]]);
        const i128 link = 2 * row - (i128)((int64_t)fr[link_f[l]] * (int64_t)sr[r[l]]);
        rec[l] = ParafitRecord{(uint64_t)link, (int64_t)(link >> 64), (uint64_t)row, (int64_t)(row >> 64)};
        total += row;
    }
}

void parafit_host(const int32_t *g_f, const int32_t *g_s, const ParafitPlan &P, const int32_t *link_f, const int32_t *link_s, uint64_t seed,
                  st_parafit_sum *total, st_parafit_sum *link_obs, int64_t *link_n_ge, st_parafit_sum *link_all)
{
    const size_t L = (size_t)P.n_links;
    std::vector<int32_t> r(L);
    std::vector<ParafitRecord> rec(L);
    std::vector<i128> obs(L);
    std::fill(link_n_ge, link_n_ge + L, (int64_t)0);
    for (int64_t p = 0; p < P.rows; p++) {
        parafit_relabel(P, link_s, seed, p, r.data());
        i128 t;
        parafit_records(g_f, g_s, P, link_f, r.data(), rec.data(), t);
        total[p] = parafit_sum(t);
        for (size_t l = 0; l < L; l++) {
            const i128 v = parafit_i128(rec[l].link_lo, rec[l].link_hi);
            if (p == 0) {
                obs[l] = v;
                link_obs[l] = parafit_sum(v);
            } else if (v >= obs[l]) {
                link_n_ge[l]++;
            }
            if (link_all) link_all[(size_t)p * L + l] = parafit_sum(v);
        }
    }
}

}  // namespace st
