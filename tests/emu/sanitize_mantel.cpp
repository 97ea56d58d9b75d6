// The host side of the Mantel sums (suchtree_amd/csrc/mantel_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_mantel_host.py builds this with -fsanitize=address,undefined): the plan on both forms -- the wave form up to
// 64 rows, the row pairs above, chunk cuts that tile every block of permutations once -- the invariant sums and the
// restatement against a plain loop over the definition, the 128-bit carry at the largest codes, the quantiser on its
// rounding edge, and every argument error in the stated order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/mantel_plan.h"
#include "chunks_tile.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 2525;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Case {
    int32_t n = 0;
    std::vector<int32_t> x, y, z;
};

static Case make_case(int32_t n, bool extreme)
{
    Case C;
    C.n = n;
    const size_t m = (size_t)n * (size_t)(n - 1) / 2;
    C.x.assign((size_t)n * (size_t)n, 0);
    C.y.resize(m);
    C.z.resize(m);
    auto draw = [&]() { return extreme ? ((rnd() & 1) ? INT32_MAX : -INT32_MAX) : (int32_t)(rnd() >> 32); };
    size_t k = 0;
    for (int32_t i = 0; i < n; i++) {
        C.x[(size_t)i * n + i] = (int32_t)rnd();      // (the diagonal is ignored)
        for (int32_t j = 0; j < i; j++, k++) {
            C.x[(size_t)i * n + j] = C.x[(size_t)j * n + i] = draw();
            C.y[k] = draw();
            C.z[k] = draw();
        }
    }
    return C;
}

static i128 of(uint64_t lo, int64_t hi) { return (i128)(((unsigned __int128)(uint64_t)hi << 64) | lo); }

static int check_case(const Case &C, bool partial, int64_t perms, int64_t chunk, uint64_t seed, int32_t stream)
{
    std::string err;
    MantelPlan P;
    st_mantel_moments M;
    std::vector<st_mantel_sums> out((size_t)perms + 1);
    const int32_t *z = partial ? C.z.data() : nullptr;
    CHECK(mantel_plan(C.x.data(), C.y.data(), z, C.n, perms, stream, chunk, &M, out.data(), P, err) == ST_OK);
    const int32_t n = C.n;
    CHECK(P.n == n && P.rows == perms + 1 && P.partial == partial && P.wave == (n <= kMantelWaveMax));
    CHECK(P.items == (P.wave ? 1 : (n + 1) / 2));
    // the chunks tile every block once, in order
    if (chunks_tile(P, chunk, [&](int64_t n_perms) { return P.items * n_perms; })) return 1;
    // the invariant sums
    i128 sx = 0, sy = 0, sz = 0, sxx = 0, syy = 0, szz = 0, syz = 0;
    size_t k = 0;
    for (int32_t i = 0; i < n; i++)
        for (int32_t j = 0; j < i; j++, k++) {
            const i128 xv = C.x[(size_t)i * n + j], yv = C.y[k], zv = partial ? C.z[k] : 0;
            sx += xv, sy += yv, sz += zv, sxx += xv * xv, syy += yv * yv, szz += zv * zv, syz += yv * zv;
        }
    CHECK(of(M.sx_lo, M.sx_hi) == sx && of(M.sy_lo, M.sy_hi) == sy && of(M.sz_lo, M.sz_hi) == sz);
    CHECK(of(M.sxx_lo, M.sxx_hi) == sxx && of(M.syy_lo, M.syy_hi) == syy && of(M.szz_lo, M.szz_hi) == szz && of(M.syz_lo, M.syz_hi) == syz);
    // the restatement against the definition, the pairs in another order
    mantel_host(C.x.data(), C.y.data(), z, P, seed, stream, out.data());
    std::vector<int32_t> sigma((size_t)n);
    for (int64_t p = 0; p <= perms; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        if (p == 0)
            for (int32_t i = 0; i < n; i++) CHECK(sigma[(size_t)i] == i);
        i128 sxy = 0, sxz = 0;
        for (int32_t j = 0; j < n; j++)
            for (int32_t i = n - 1; i > j; i--) {
                const size_t kk = (size_t)i * (size_t)(i - 1) / 2 + (size_t)j;
                const i128 xv = C.x[(size_t)sigma[(size_t)j] * n + sigma[(size_t)i]];      // (the mirror cell: x_sq is symmetric)
                sxy += xv * C.y[kk];
                if (partial) sxz += xv * C.z[kk];
            }
        CHECK(of(out[(size_t)p].sxy_lo, out[(size_t)p].sxy_hi) == sxy);
        CHECK(of(out[(size_t)p].sxz_lo, out[(size_t)p].sxz_hi) == sxz);
    }
    return 0;
}

static int check_carry()
{
    // n = 65, every code 2^31 - 1 on both sides: 2080 pairs of (2^31 - 1)^2, past 2^63
    Case C = make_case(65, true);
    for (auto &v : C.x) v = INT32_MAX;
    for (auto &v : C.y) v = INT32_MAX;
    for (auto &v : C.z) v = -INT32_MAX;
    std::string err;
    MantelPlan P;
    st_mantel_moments M;
    st_mantel_sums out[3];
    CHECK(mantel_plan(C.x.data(), C.y.data(), C.z.data(), 65, 2, 0, 0, &M, out, P, err) == ST_OK);
    mantel_host(C.x.data(), C.y.data(), C.z.data(), P, 9, 0, out);
    const i128 one = (i128)INT32_MAX * INT32_MAX * 2080;
    CHECK(one > (i128)INT64_MAX);
    for (int p = 0; p < 3; p++) CHECK(of(out[p].sxy_lo, out[p].sxy_hi) == one && of(out[p].sxz_lo, out[p].sxz_hi) == -one);
    CHECK(of(M.sxx_lo, M.sxx_hi) == one && of(M.syz_lo, M.syz_hi) == -one);
    return 0;
}

// the default block (chunk_tasks 0) where each of its two bounds binds, with more permutations than the bound
static int check_blocks()
{
    struct Want {
        int32_t n;
        int64_t perm_block;
    };
    for (const Want w : {Want{64, 524288} /* the sigma rows: 2^26 / (2 x 64) */, Want{65, 127100} /* the partial records: 2^22 / 33 row pairs */}) {
        const Case C = make_case(w.n, false);
        std::string err;
        MantelPlan P;
        st_mantel_moments M;
        st_mantel_sums out;
        CHECK(mantel_plan(C.x.data(), C.y.data(), nullptr, w.n, 600000, 0, 0, &M, &out, P, err) == ST_OK);
        CHECK(P.perm_block == w.perm_block);
        CHECK(w.perm_block == std::min(kDispersionSigmaBytes / (2 * w.n), kMantelBlockTasks / P.items));
        if (chunks_tile(P, 0, [&](int64_t n_perms) { return P.items * n_perms; })) return 1;
    }
    return 0;
}

static int check_quantise()
{
    std::string err;
    int32_t s = 0;
    std::vector<double> v{0.0, -0.0, 1.0, -3.75, 0.1, 1e-9};
    std::vector<int32_t> q(v.size());
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_OK);
    CHECK(s == 29);      // (3.75 in [2, 4): ilogb 1)
    for (size_t k = 0; k < v.size(); k++) CHECK(q[k] == (int32_t)std::llrint(std::ldexp(v[k], s)));
    CHECK(std::abs((int64_t)q[3]) >= ((int64_t)1 << 30) && std::abs((int64_t)q[3]) < ((int64_t)1 << 31));
    // a top that would round up to 2^31: one shift less, and it lands on 2^30
    const double edge = std::nextafter(2.0, 0.0);
    CHECK(mantel_quantise(&edge, 1, ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_OK && s == 29 && q[0] == (1 << 30));
    // large and tiny values take negative and large shifts
    const double big = 3e200, tiny = 3e-200;
    CHECK(mantel_quantise(&big, 1, ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_OK && s < 0 && q[0] >= (1 << 30));
    CHECK(mantel_quantise(&tiny, 1, ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_OK && s > 600 && q[0] >= (1 << 30));
    const double zeros[2] = {0.0, -0.0};
    CHECK(mantel_quantise(zeros, 2, ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_OK && s == 0 && q[0] == 0 && q[1] == 0);
    CHECK(mantel_quantise(nullptr, 0, ST_MANTEL_SHIFT_AUTO, nullptr, &s, err) == ST_OK && s == 0);
    // a caller's shift
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), 4, q.data(), &s, err) == ST_OK && s == 4 && q[3] == -60 && q[4] == 2);
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), 30, q.data(), &s, err) == ST_ERR_ARG && err.find("2^31") != std::string::npos);
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), 2001, q.data(), &s, err) == ST_ERR_ARG);
    CHECK(mantel_quantise(v.data(), -1, 0, q.data(), &s, err) == ST_ERR_ARG);
    CHECK(mantel_quantise(nullptr, 2, 0, q.data(), &s, err) == ST_ERR_ARG);
    v[4] = std::numeric_limits<double>::quiet_NaN();
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), ST_MANTEL_SHIFT_AUTO, q.data(), &s, err) == ST_ERR_ARG && err.find("v[4]") != std::string::npos);
    v[1] = -std::numeric_limits<double>::infinity();
    CHECK(mantel_quantise(v.data(), (int64_t)v.size(), 0, q.data(), &s, err) == ST_ERR_ARG && err.find("v[1]") != std::string::npos);
    return 0;
}

static int check_errors()
{
    Case C = make_case(5, false);
    std::string err;
    MantelPlan P;
    st_mantel_moments M;
    st_mantel_sums out[4];
    auto plan = [&](const int32_t *x, const int32_t *y, int32_t n, int64_t perms, int32_t stream, int64_t chunk, st_mantel_moments *m, st_mantel_sums *o) {
        return mantel_plan(x, y, nullptr, n, perms, stream, chunk, m, o, P, err);
    };
    const int32_t *x = C.x.data(), *y = C.y.data();
    CHECK(plan(nullptr, nullptr, 2, -1, -1, -1, nullptr, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, kPermMaxUniverse + 1, -1, -1, -1, nullptr, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, 5, -1, -1, -1, nullptr, nullptr) == ST_ERR_ARG && err == "permutations < 0");
    CHECK(plan(nullptr, nullptr, 5, 3, -1, -1, nullptr, nullptr) == ST_ERR_ARG && err == "chunk_tasks < 0");
    CHECK(plan(nullptr, nullptr, 5, 3, -1, 0, nullptr, nullptr) == ST_ERR_ARG && err == "stream < 0");
    CHECK(plan(nullptr, nullptr, 5, (int64_t)1 << 31, 0, 0, nullptr, nullptr) == ST_ERR_ARG && err.find("permutations") != std::string::npos);
    CHECK(plan(nullptr, y, 5, 3, 0, 0, nullptr, nullptr) == ST_ERR_ARG && err == "x_sq or y is NULL");
    CHECK(plan(x, nullptr, 5, 3, 0, 0, nullptr, nullptr) == ST_ERR_ARG && err == "x_sq or y is NULL");
    CHECK(plan(x, y, 5, 3, 0, 0, nullptr, out) == ST_ERR_ARG && err == "moments or out is NULL");
    CHECK(plan(x, y, 5, 3, 0, 0, &M, nullptr) == ST_ERR_ARG && err == "moments or out is NULL");
    Case A = C;
    A.x[3 * 5 + 1] ^= 1;      // (3, 1) and its mirror (1, 3): the first in row-major order is [1][3]
    A.x[4 * 5 + 2] ^= 1;
    CHECK(plan(A.x.data(), y, 5, 3, 0, 0, &M, out) == ST_ERR_ARG && err.find("x_sq[1][3]") != std::string::npos);
    CHECK(plan(x, y, 5, 3, 0, 0, &M, out) == ST_OK);
    return 0;
}

int main()
{
    for (int32_t n : {3, 4, 5, 63, 64, 65, 66, 129, 257})
        for (int partial = 0; partial < 2; partial++) {
            const Case C = make_case(n, false);
            if (check_case(C, partial != 0, n > 100 ? 2 : 5, 0, rnd(), (int32_t)(rnd() % 1000))) return 1;
            if (check_case(C, partial != 0, 7, n > 64 ? 16 : 3, rnd(), 0)) return 1;
        }
    if (check_case(make_case(65, true), true, 3, 1, 11, 0)) return 1;
    if (check_blocks() || check_carry() || check_quantise() || check_errors()) return 1;
    std::printf("sanitize mantel ok\n");
    return 0;
}
