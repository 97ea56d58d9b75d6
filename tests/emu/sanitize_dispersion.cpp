// The host side of the partner-dispersion reduction (suchtree_amd/csrc/dispersion_plan.cpp) under AddressSanitizer +
// UBSan (tests/test_dispersion_host.py builds this with -fsanitize=address,undefined): the plan on the size-class
// edges -- order, class ranges, chunk cuts that tile every block of permutations once -- the scatter, the restatement
// against a plain loop on those edges, the special values of the comparison rule, and every argument error.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/dispersion_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 777;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Case {
    int32_t n = 0;
    std::vector<int32_t> pos;
    std::vector<int64_t> off{0};
};

static void add_set(Case &C, int k)      // k distinct positions of the universe, increasing
{
    std::vector<int32_t> all((size_t)C.n);
    for (int32_t i = 0; i < C.n; i++) all[(size_t)i] = i;
    for (int i = 0; i < k; i++) std::swap(all[(size_t)i], all[(size_t)i + rnd() % (uint64_t)(C.n - i)]);
    std::sort(all.begin(), all.begin() + k);
    C.pos.insert(C.pos.end(), all.begin(), all.begin() + k);
    C.off.push_back((int64_t)C.pos.size());
}

static int plan_of(const Case &C, int64_t perms, int64_t chunk, DispersionPlan &P, std::string &err, int32_t stream = 0)
{
    return dispersion_plan(C.n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), (int64_t)C.off.size() - 1, perms, stream, chunk, P, err);
}

static bool same(const st_dispersion_record &a, const st_dispersion_record &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int check_case(const Case &C, int64_t perms)
{
    std::string err;
    DispersionPlan P;
    CHECK(plan_of(C, perms, 0, P, err) == ST_OK);
    const int64_t n_sets = (int64_t)C.off.size() - 1, R = perms + 1;
    CHECK(P.rows == R && P.n_sets == n_sets && P.order.size() == P.sets.size());
    // the order: live sets only, by class, by index within a class; the class ranges
    int64_t live = 0;
    for (int64_t r = 0; r < n_sets; r++) live += C.off[(size_t)r + 1] - C.off[(size_t)r] >= 2;
    CHECK((int64_t)P.order.size() == live && P.class_begin[0] == 0 && P.class_begin[kDispersionClasses] == live);
    for (int64_t c = 0; c < live; c++) {
        const int64_t r = P.order[(size_t)c];
        const int k = (int)(C.off[(size_t)r + 1] - C.off[(size_t)r]);
        CHECK(P.sets[(size_t)c].begin == C.off[(size_t)r] && P.sets[(size_t)c].count == k && k <= P.max_count);
        const int cls = dispersion_class(k);
        CHECK(cls >= 0 && cls < kDispersionClasses && P.class_begin[cls] <= c && c < P.class_begin[cls + 1]);
        CHECK(k > kDispersionWaveMax ? cls == 6 : (dispersion_lanes(k) == 2 << cls && dispersion_lanes(k) >= k && (k <= 2 || dispersion_lanes(k) < 2 * k)));
        if (c > 0) {
            const int64_t q = P.order[(size_t)c - 1];
            const int pc = dispersion_class((int)(C.off[(size_t)q + 1] - C.off[(size_t)q]));
            CHECK(pc < cls || (pc == cls && q < r));
        }
    }
    // chunks tile every block's tasks once, in order; the scatter puts task t where (set, p) belongs
    std::vector<float> D((size_t)C.n * (size_t)C.n);
    for (auto &v : D) v = (float)(rnd() % 4096) / 64.0f;
    std::vector<st_dispersion_record> want((size_t)(n_sets * R));
    dispersion_host(D.data(), P, C.pos.data(), C.off.data(), 99, 5, want.data());
    for (int64_t cb : {1, 2, 7, 0}) {
        DispersionPlan Q;
        CHECK(plan_of(C, perms, cb, Q, err) == ST_OK);
        CHECK(Q.perm_block >= 1 && Q.perm_block <= R && (cb == 0 || Q.perm_block <= cb));
        std::vector<st_dispersion_record> got((size_t)(n_sets * R), st_dispersion_record{0.0, 0.0});
        int64_t p_next = 0, t_next = 0;
        for (const DispersionChunk &k : Q.chunks) {
            if (t_next == 0) CHECK(k.p_begin == p_next && k.n_perms == std::min(Q.perm_block, R - p_next));
            CHECK(k.task_begin == t_next && k.n_tasks >= 1 && k.n_tasks <= Q.max_chunk_tasks && (cb == 0 || k.n_tasks <= cb));
            // a chunk's records as the device would leave them: task t = c * n_perms + (p - p0)
            std::vector<st_dispersion_record> rec((size_t)k.n_tasks);
            for (int64_t j = 0; j < k.n_tasks; j++) {
                const int64_t t = k.task_begin + j, c = t / k.n_perms, p = k.p_begin + t % k.n_perms;
                rec[(size_t)j] = want[(size_t)(Q.order[(size_t)c] * R + p)];
            }
            dispersion_scatter(Q, k, rec.data(), got.data());
            t_next += k.n_tasks;
            if (t_next == live * k.n_perms) {
                t_next = 0;
                p_next += k.n_perms;
            }
        }
        CHECK(live == 0 ? Q.chunks.empty() : (t_next == 0 && p_next == R));
        for (size_t i = 0; i < got.size(); i++) CHECK(same(got[i], want[i]));
    }
    // the restatement against a plain loop: long double sums, the minimum by std::min
    std::vector<int32_t> sigma((size_t)C.n);
    for (int64_t p = 0; p < R; p++) {
        perm_host(99, 5, p, 0, C.n, sigma.data());
        for (int64_t r = 0; r < n_sets; r++) {
            const int64_t b = C.off[(size_t)r], k = C.off[(size_t)r + 1] - b;
            long double pair = 0, nearest = 0;
            for (int64_t i = 0; i < k && k >= 2; i++) {
                float m = std::numeric_limits<float>::infinity();
                for (int64_t j = 0; j < k; j++) {
                    if (j == i) continue;
                    const float v = D[(size_t)sigma[(size_t)C.pos[(size_t)(b + i)]] * (size_t)C.n + (size_t)sigma[(size_t)C.pos[(size_t)(b + j)]]];
                    pair += v;
                    m = std::min(m, v);
                }
                nearest += m;
            }
            const st_dispersion_record &g = want[(size_t)(r * R + p)];
            CHECK(std::fabs((double)(pair - g.pair_sum)) <= (double)(k * k) * 0x1p-52 * (double)pair);
            CHECK(std::fabs((double)(nearest - g.nearest_sum)) <= (double)k * 0x1p-52 * (double)nearest);
        }
    }
    return 0;
}

int main()
{
    for (int32_t n : {3, 64, 65, 700}) {
        Case C;
        C.n = n;
        for (int k : {0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 700})
            if (k <= n) add_set(C, k);
        add_set(C, 2);      // a second set of the first class, behind the others
        if (check_case(C, n > 100 ? 2 : 5)) return 1;
    }
    {      // nothing to do: no sets, and only sets of fewer than two positions
        Case C;
        C.n = 5;
        if (check_case(C, 3)) return 1;
        add_set(C, 1);
        add_set(C, 0);
        if (check_case(C, 3)) return 1;
    }
    {      // the comparison rule on special values: a NaN is never taken, +inf only if nothing is smaller, the first of equals stays
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const int32_t q[3] = {0, 1, 2};
        float D[9] = {0, nan, 2.0f, inf, 0, inf, -0.0f, 0.0f, 0};
        const st_dispersion_record r = dispersion_record(D, 3, q, 3);
        CHECK(std::isnan(r.pair_sum));                          // row 0 sums a NaN
        CHECK(r.nearest_sum == inf);                            // 2 (row 0: the NaN is skipped) + inf (row 1) + -0.0 (row 2)
        float E[9] = {0, nan, nan, 1.0f, 0, 3.0f, -0.0f, 0.0f, 0};
        const st_dispersion_record s = dispersion_record(E, 3, q, 3);
        CHECK(s.nearest_sum == inf);                            // row 0 has only NaN: its minimum stays +inf
        float F[4] = {0, -0.0f, 0.0f, 0};
        const int32_t q2[2] = {0, 1};
        const st_dispersion_record z = dispersion_record(F, 2, q2, 2);
        CHECK(z.pair_sum == 0.0 && z.nearest_sum == 0.0 && !std::signbit(z.nearest_sum));      // -0.0 + +0.0
        const st_dispersion_record one = dispersion_record(F, 2, q2, 1);
        CHECK(one.pair_sum == 0.0 && one.nearest_sum == 0.0);
    }
    // arguments
    {
        Case good;
        good.n = 40;
        for (int k : {3, 7, 40, 1}) add_set(good, k);
        std::string err;
        DispersionPlan P;
        CHECK(plan_of(good, 5, 0, P, err) == ST_OK);
        CHECK(plan_of(good, -1, 0, P, err) == ST_ERR_ARG && !err.empty());      // negative permutations
        CHECK(plan_of(good, 5, -1, P, err) == ST_ERR_ARG);                      // negative chunk_tasks
        CHECK(plan_of(good, 5, 0, P, err, -1) == ST_ERR_ARG);                   // negative stream
        Case c = good;
        c.n = 2;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // a universe below 3 ...
        c.n = kPermMaxUniverse + 1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // ... and above the limit
        c.n = kPermMaxUniverse;
        CHECK(plan_of(c, 5, 0, P, err) == ST_OK);
        c = good;
        c.pos[1] = 40;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // a position outside the universe
        c.pos[1] = -1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);
        c = good;
        std::swap(c.pos[3], c.pos[4]);
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG && err.find("increasing") != std::string::npos);      // an unsorted set
        c = good;
        c.pos[4] = c.pos[3];
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // a duplicate
        c = good;
        c.off[2] = c.off[1] - 1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // offsets that go back
        c = good;
        c.off.back() += 1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                          // offsets past the positions
        CHECK(dispersion_plan(40, nullptr, 3, good.off.data(), 1, 5, 0, 0, P, err) == ST_ERR_ARG);      // NULL arrays
        CHECK(dispersion_plan(40, good.pos.data(), 3, nullptr, 1, 5, 0, 0, P, err) == ST_ERR_ARG);
        CHECK(dispersion_plan(40, nullptr, 0, nullptr, 0, 5, 0, 0, P, err) == ST_OK && P.chunks.empty());
    }
    std::printf("sanitize dispersion ok\n");
    return 0;
}
