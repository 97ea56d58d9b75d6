// The host side of ParaFit (suchtree_amd/csrc/parafit_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_parafit_host.py builds this with -fsanitize=address,undefined): the plan on both forms -- the wave form up
// to 64 links over 64 S positions, the link rows above, chunk cuts that tile every block of permutations once -- the
// restatement against a plain loop over the definition, the 128-bit carry at the largest codes, distinct images for the
// links of one F position, and every argument error in the stated order.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/parafit_plan.h"
#include "chunks_tile.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 4242;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Case {
    int32_t n_f = 0, n_s = 0, L = 0;
    std::vector<int32_t> g_f, g_s, link_f, link_s, stream;
};

static std::vector<int32_t> symmetric(int32_t n, bool extreme)
{
    std::vector<int32_t> g((size_t)n * (size_t)n);
    for (int32_t i = 0; i < n; i++)
        for (int32_t j = 0; j <= i; j++)
            g[(size_t)i * n + j] = g[(size_t)j * n + i] = extreme ? ((rnd() & 1) ? INT32_MAX : -INT32_MAX) : (int32_t)(rnd() >> 32);
    return g;
}

static Case make_case(int32_t n_f, int32_t n_s, int32_t L, bool extreme)
{
    Case C;
    C.n_f = n_f;
    C.n_s = n_s;
    C.L = L;
    C.g_f = symmetric(n_f, extreme);
    C.g_s = symmetric(n_s, extreme);
    std::set<int64_t> cells;
    while ((int32_t)cells.size() < L) cells.insert((int64_t)(rnd() % ((uint64_t)n_f * (uint64_t)n_s)));
    for (const int64_t c : cells) {      // (ascending cells: (f, s) order)
        C.link_f.push_back((int32_t)(c / n_s));
        C.link_s.push_back((int32_t)(c % n_s));
    }
    for (int32_t i = 0; i < n_f; i++) C.stream.push_back(100 + i);
    return C;
}

static int check_case(const Case &C, int64_t perms, int64_t chunk, uint64_t seed)
{
    std::string err;
    ParafitPlan P;
    const size_t L = (size_t)C.L, R = (size_t)perms + 1;
    std::vector<st_parafit_sum> total(R), obs(L), every(R * L);
    std::vector<int64_t> n_ge(L, -1);
    CHECK(parafit_plan(C.g_f.data(), C.n_f, C.g_s.data(), C.n_s, C.link_f.data(), C.link_s.data(), C.L, C.stream.data(), perms, chunk, total.data(),
                       obs.data(), n_ge.data(), P, err) == ST_OK);
    CHECK(P.wave == (C.L <= 64 && C.n_s <= 64) && P.items == (P.wave ? 1 : C.L) && P.rows == perms + 1);
    // the groups partition the links by F position
    int32_t at = 0;
    for (const ParafitGroup &g : P.groups) {
        CHECK(g.begin == at && g.count > 0 && g.stream == C.stream[(size_t)g.f]);
        for (int32_t l = g.begin; l < g.begin + g.count; l++) CHECK(C.link_f[(size_t)l] == g.f);
        at += g.count;
    }
    CHECK(at == C.L);
    // the chunks tile every block once
    if (chunks_tile(P, chunk, [&](int64_t n_perms) { return P.items * n_perms; })) return 1;
    parafit_host(C.g_f.data(), C.g_s.data(), P, C.link_f.data(), C.link_s.data(), seed, total.data(), obs.data(), n_ge.data(), every.data());
    // a plain loop over the definition
    std::vector<int32_t> r(L), sigma((size_t)C.n_s);
    std::vector<i128> first(L);
    std::vector<int64_t> want_ge(L, 0);
    for (int64_t p = 0; p <= perms; p++) {
        for (size_t l = 0; l < L; l++) {
            perm_host(seed, C.stream[(size_t)C.link_f[l]], p, 0, C.n_s, sigma.data());
            r[l] = sigma[(size_t)C.link_s[l]];
        }
        for (size_t l = 1; l < L; l++)
            if (C.link_f[l] == C.link_f[l - 1]) CHECK(r[l] != r[l - 1]);      // (distinct images under one F position)
        i128 sum = 0;
        for (size_t l = 0; l < L; l++) {
            i128 row = 0, diag = 0;
            for (size_t k = 0; k < L; k++) {
                const i128 t = (i128)C.g_f[(size_t)C.link_f[l] * C.n_f + C.link_f[k]] * (i128)C.g_s[(size_t)r[l] * C.n_s + r[k]];
                row += t;
                if (k == l) diag = t;
            }
            sum += row;
            const i128 link = 2 * row - diag;
            const st_parafit_sum &got = every[(size_t)p * L + l];
            CHECK(parafit_i128(got.lo, got.hi) == link);
            if (p == 0) {
                first[l] = link;
                CHECK(parafit_i128(obs[l].lo, obs[l].hi) == link);
            } else if (link >= first[l]) {
                want_ge[l]++;
            }
        }
        CHECK(parafit_i128(total[(size_t)p].lo, total[(size_t)p].hi) == sum);
    }
    CHECK(want_ge == n_ge);
    return 0;
}

// the default block (chunk_tasks 0), with more permutations than its bound: the link records' bound, 2^22 / L, binds at
// every L (the R rows' is 2^26 / (2 L)), in the wave form and in the row form
static int check_blocks()
{
    for (const int32_t n_s : {3, 65}) {
        const Case C = make_case(3, n_s, 3, false);
        std::string err;
        ParafitPlan P;
        st_parafit_sum total, obs;
        int64_t n_ge = 0;
        CHECK(parafit_plan(C.g_f.data(), 3, C.g_s.data(), n_s, C.link_f.data(), C.link_s.data(), 3, C.stream.data(), 1500000, 0, &total, &obs, &n_ge, P, err) ==
              ST_OK);
        CHECK(P.wave == (n_s <= kParafitWaveMax) && P.perm_block == 1398101);
        CHECK(P.perm_block == std::min(kDispersionSigmaBytes / (2 * 3), kParafitBlockTasks / 3));
        if (chunks_tile(P, 0, [&](int64_t n_perms) { return P.items * n_perms; })) return 1;
    }
    return 0;
}

static int check_errors()
{
    Case C = make_case(5, 6, 7, false);
    std::string err;
    ParafitPlan P;
    std::vector<st_parafit_sum> total(2), obs(7);
    std::vector<int64_t> n_ge(7);
    auto plan = [&](const Case &K, int64_t perms, int64_t chunk, bool in = true, bool out = true) {
        return parafit_plan(in ? K.g_f.data() : nullptr, K.n_f, K.g_s.data(), K.n_s, K.link_f.data(), K.link_s.data(), K.L, K.stream.data(), perms, chunk,
                            out ? total.data() : nullptr, obs.data(), n_ge.data(), P, err);
    };
    auto has = [&](const char *text) { return err.find(text) != std::string::npos; };
    Case K = C;
    K.n_f = 2;
    K.n_s = 2;
    CHECK(plan(K, -1, -1, false, false) == ST_ERR_ARG && has("n_f = 2"));
    K.n_f = 5;
    K.L = 2;
    CHECK(plan(K, -1, -1, false, false) == ST_ERR_ARG && has("n_s = 2"));
    K.n_s = 6;
    CHECK(plan(K, -1, -1, false, false) == ST_ERR_ARG && has("n_links = 2"));
    K.L = 16385;
    CHECK(plan(K, -1, -1, false, false) == ST_ERR_ARG && has("n_links = 16385"));
    K.L = 7;
    CHECK(plan(K, -1, 0, false, false) == ST_ERR_ARG && has("< 0"));
    CHECK(plan(K, 0, -1, false, false) == ST_ERR_ARG && has("< 0"));
    CHECK(plan(K, (int64_t)1 << 31, 0, false, false) == ST_ERR_ARG && has("2^31 - 1"));
    CHECK(plan(K, 1, 0, false, false) == ST_ERR_ARG && has("g_f, g_s"));
    CHECK(plan(K, 1, 0, true, false) == ST_ERR_ARG && has("total, link_obs"));
    K.link_s[3] = 6;
    K.link_f[5] = -1;
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("link 3 ") && has("S position"));
    K.link_s[3] = C.link_s[3];
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("link 5 ") && has("F position"));
    K = C;
    std::swap(K.link_f[2], K.link_f[4]);
    std::swap(K.link_s[2], K.link_s[4]);
    K.stream[0] = -1;
    K.g_f[1 * 5 + 3] ^= 1;
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("strictly increasing"));
    K.link_f = C.link_f;
    K.link_s = C.link_s;
    K.link_f[4] = K.link_f[3];
    K.link_s[4] = K.link_s[3];
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("link 4 ") && has("strictly increasing"));      // (a repeated link)
    K.link_f = C.link_f;
    K.link_s = C.link_s;
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("stream_f[0]"));
    K.stream[0] = 0;
    K.g_s[2 * 6 + 5] ^= 1;
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("g_f is not symmetric: g_f[1][3]"));
    K.g_f = C.g_f;
    CHECK(plan(K, 1, 0) == ST_ERR_ARG && has("g_s is not symmetric: g_s[2][5]"));
    CHECK(plan(C, 1, 0) == ST_OK);
    return 0;
}

int main()
{
    for (const auto &shape : {std::vector<int>{3, 3, 3}, {64, 64, 64}, {5, 64, 63}, {9, 65, 40}, {40, 3, 65}, {30, 70, 129}})
        for (const int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)70})
            if (check_case(make_case(shape[0], shape[1], shape[2], false), 5, chunk, 99 + (uint64_t)chunk)) return 1;
    if (check_case(make_case(20, 66, 257, true), 2, 0, 5)) return 1;      // 257^2 terms of +-(2^31 - 1)^2: past 64 bits
    if (check_blocks() || check_errors()) return 1;
    std::printf("sanitize parafit ok\n");
    return 0;
}
