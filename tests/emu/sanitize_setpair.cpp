// The host side of the between-set dispersion reduction (suchtree_amd/csrc/setpair_plan.cpp) under AddressSanitizer +
// UBSan (tests/test_beta_dispersion_host.py builds this with -fsanitize=address,undefined): the plan on the size-class
// edges -- order by (class of k_r, k_c, direction), class ranges, chunk cuts that tile every block of permutations once --
// over whole triangles and ranges cut mid-row, the scatter, the restatement against a plain loop, the structural no-entry
// rule, the special values of the comparison rule, and every argument error in the stated order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/setpair_plan.h"

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

static int plan_of(const Case &C, int64_t begin, int64_t count, int exclude, int64_t perms, int64_t chunk, SetpairPlan &P, std::string &err,
                   int32_t stream = 0)
{
    return setpair_plan(C.n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), (int64_t)C.off.size() - 1, begin, count, exclude, perms, stream, chunk,
                        P, err);
}

static bool same(const st_dispersion_record &a, const st_dispersion_record &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int check_case(const Case &C, int64_t begin, int64_t count, int exclude, int64_t perms)
{
    std::string err;
    SetpairPlan P;
    CHECK(plan_of(C, begin, count, exclude, perms, 0, P, err) == ST_OK);
    const int64_t R = perms + 1, dirs = 2 * count;
    CHECK(P.rows == R && P.begin == begin && P.count == count && P.order.size() == P.tasks.size() && P.exclude == (exclude != 0));
    // the direction table: u = (k - begin) * 2 + dir, pair k = i (i - 1) / 2 + j
    std::vector<int64_t> set_r((size_t)dirs), set_c((size_t)dirs);
    for (int64_t k = 0; k < count; k++) {
        int64_t i, j;
        unifrac_pair(begin + k, i, j);
        CHECK(j >= 0 && j < i && i * (i - 1) / 2 + j == begin + k);
        set_r[(size_t)(2 * k)] = set_c[(size_t)(2 * k + 1)] = i;
        set_c[(size_t)(2 * k)] = set_r[(size_t)(2 * k + 1)] = j;
    }
    auto size = [&](int64_t r) { return (int)(C.off[(size_t)r + 1] - C.off[(size_t)r]); };
    int64_t live = 0;
    for (int64_t u = 0; u < dirs; u++) live += size(set_r[(size_t)u]) >= 1 && size(set_c[(size_t)u]) >= 1;
    CHECK((int64_t)P.order.size() == live && P.class_begin[0] == 0 && P.class_begin[kDispersionClasses] == live);
    int max_walk = 0;
    for (int64_t c = 0; c < live; c++) {
        const int64_t u = P.order[(size_t)c];
        const SetpairTaskDev &t = P.tasks[(size_t)c];
        CHECK(u >= 0 && u < dirs && t.r_begin == C.off[(size_t)set_r[(size_t)u]] && t.r_count == size(set_r[(size_t)u]));
        CHECK(t.c_begin == C.off[(size_t)set_c[(size_t)u]] && t.c_count == size(set_c[(size_t)u]) && t.r_count >= 1 && t.c_count >= 1);
        const int cls = dispersion_class(t.r_count);
        CHECK(cls >= 0 && cls < kDispersionClasses && P.class_begin[cls] <= c && c < P.class_begin[cls + 1]);
        CHECK(t.r_count > kDispersionWaveMax ? cls == 6 : (dispersion_lanes(t.r_count) == 2 << cls && dispersion_lanes(t.r_count) >= t.r_count));
        if (cls == 6) max_walk = std::max(max_walk, t.c_count);
        if (c > 0) {
            const SetpairTaskDev &b = P.tasks[(size_t)c - 1];
            const int pc = dispersion_class(b.r_count);
            CHECK(pc < cls || (pc == cls && (b.c_count < t.c_count || (b.c_count == t.c_count && P.order[(size_t)c - 1] < u))));
        }
    }
    CHECK(P.max_walk == max_walk);
    // chunks tile every block's tasks once, in order; the scatter puts task t where (direction, p) belongs
    std::vector<float> D((size_t)C.n * (size_t)C.n);
    for (auto &v : D) v = (float)(rnd() % 4096) / 64.0f;
    std::vector<st_dispersion_record> want((size_t)std::max<int64_t>(dirs * R, 1));
    setpair_host(D.data(), P, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), 99, 5, want.data());
    for (int64_t cb : {1, 2, 7, 0}) {
        SetpairPlan Q;
        CHECK(plan_of(C, begin, count, exclude, perms, cb, Q, err) == ST_OK);
        CHECK(Q.perm_block >= 1 && Q.perm_block <= R && (cb == 0 || Q.perm_block <= cb));
        std::vector<st_dispersion_record> got((size_t)std::max<int64_t>(dirs * R, 1), st_dispersion_record{0.0, 0.0});
        int64_t p_next = 0, t_next = 0;
        for (const DispersionChunk &k : Q.chunks) {
            if (t_next == 0) CHECK(k.p_begin == p_next && k.n_perms == std::min(Q.perm_block, R - p_next));
            CHECK(k.task_begin == t_next && k.n_tasks >= 1 && k.n_tasks <= Q.max_chunk_tasks && (cb == 0 || k.n_tasks <= cb));
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
        for (int64_t x = 0; x < dirs * R; x++) {      // (a direction without a task: zeros on both sides)
            if (!same(got[(size_t)x], want[(size_t)x])) CHECK(want[(size_t)x].pair_sum == 0.0 && want[(size_t)x].nearest_sum == 0.0);
        }
    }
    // the restatement against a plain loop: long double sums, the minimum by std::min
    std::vector<int32_t> sigma((size_t)C.n);
    for (int64_t p = 0; p < R; p++) {
        perm_host(99, 5, p, 0, C.n, sigma.data());
        for (int64_t u = 0; u < dirs; u++) {
            const int64_t br = C.off[(size_t)set_r[(size_t)u]], bc = C.off[(size_t)set_c[(size_t)u]];
            const int kr = size(set_r[(size_t)u]), kc = size(set_c[(size_t)u]);
            long double cross = 0, nearest = 0;
            for (int a = 0; a < kr; a++) {
                float m = std::numeric_limits<float>::infinity();
                bool any = false;
                for (int b = 0; b < kc; b++) {
                    if (exclude && C.pos[(size_t)(br + a)] == C.pos[(size_t)(bc + b)]) continue;
                    const float v = D[(size_t)sigma[(size_t)C.pos[(size_t)(br + a)]] * (size_t)C.n + (size_t)sigma[(size_t)C.pos[(size_t)(bc + b)]]];
                    cross += v;
                    m = std::min(m, v);
                    any = true;
                }
                if (any) nearest += m;
            }
            const st_dispersion_record &g = want[(size_t)(u * R + p)];
            CHECK(std::fabs((double)(cross - g.pair_sum)) <= (double)kr * (double)kc * 0x1p-52 * (double)cross);
            CHECK(std::fabs((double)(nearest - g.nearest_sum)) <= (double)kr * 0x1p-52 * (double)nearest);
        }
    }
    return 0;
}

// The triangle index the plans and the kernels share (plan_checks.h: unifrac_pair) where the float square root and the
// correction loops it replaced here were exact: the first 5,000 pairs and both sides of a row's first pair, up to rows
// past 2^31 (a table of more than 2^31 empty sets), where 8 k + 1 no longer fits 64 bits.
static int check_triangle_index()
{
    auto closed_form = [](int64_t k) {
        int64_t i = -1, j = -1;
        unifrac_pair(k, i, j);
        return i >= 1 && j >= 0 && j < i && j == k - i * (i - 1) / 2;
    };
    for (int64_t k = 0; k < 5000; k++) CHECK(closed_form(k));
    const int64_t two31 = (int64_t)1 << 31;
    for (int64_t i : {(int64_t)2, (int64_t)3, (int64_t)1 << 16, ((int64_t)1 << 16) + 1, two31 - 1, two31, two31 + 1}) {
        const int64_t first = i * (i - 1) / 2;
        int64_t r, j;
        unifrac_pair(first - 1, r, j);
        CHECK(r == i - 1 && j == i - 2 && closed_form(first - 1));
        unifrac_pair(first, r, j);
        CHECK(r == i && j == 0 && closed_form(first));
        unifrac_pair(first + 1, r, j);
        CHECK(r == i && j == 1 && closed_form(first + 1));
    }
    return 0;
}

int main()
{
    if (check_triangle_index()) return 1;
    for (int32_t n : {3, 64, 65, 700}) {
        Case C;
        C.n = n;
        for (int k : {0, 1, 2, 3, 8, 9, 32, 33, 64, 65, 257, 513, 700})
            if (k <= n) add_set(C, k);
        add_set(C, 2);                       // a second set of the first class, behind the others
        C.off.push_back(C.off.back());       // ... and a second empty one
        const int64_t n_sets = (int64_t)C.off.size() - 1, total = n_sets * (n_sets - 1) / 2;
        for (int exclude : {0, 1}) {
            if (check_case(C, 0, total, exclude, n > 100 ? 1 : 3)) return 1;
            if (check_case(C, 4, total - 9, exclude, 1)) return 1;      // a range that starts and ends mid-row
        }
        if (check_case(C, total, 0, 0, 2)) return 1;
        if (check_case(C, 2, 0, 1, 2)) return 1;
    }
    {      // nothing to do: no sets, one set, only empty sets
        Case C;
        C.n = 5;
        if (check_case(C, 0, 0, 0, 3)) return 1;
        add_set(C, 3);
        if (check_case(C, 0, 0, 0, 3)) return 1;
        Case E;
        E.n = 5;
        E.off = {0, 0, 0, 0};
        if (check_case(E, 0, 3, 1, 3)) return 1;
    }
    {      // the rules of one record
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const int32_t id[4] = {0, 1, 2, 3};
        float D[16] = {0, nan, 2.0f, 5.0f, inf, 0, inf, inf, -0.0f, 0.0f, 0, 1.0f, nan, nan, nan, 0};
        // {0} -> {1, 2, 3}: a NaN is summed and never taken as the minimum
        st_dispersion_record r = setpair_record(D, 4, id, id, 1, id + 1, id + 1, 3, false);
        CHECK(std::isnan(r.pair_sum) && r.nearest_sum == 2.0);
        // {3} -> {0, 1, 2}: only NaN entries, the minimum stays +inf -- an included entry, not "no entry"
        r = setpair_record(D, 4, id + 3, id + 3, 1, id, id, 3, false);
        CHECK(std::isnan(r.pair_sum) && r.nearest_sum == inf);
        // {2} -> {0, 1}: -0.0 then +0.0, the first stays; the absent lane adds +0.0
        r = setpair_record(D, 4, id + 2, id + 2, 1, id, id, 2, false);
        CHECK(r.pair_sum == 0.0 && r.nearest_sum == 0.0 && !std::signbit(r.nearest_sum));
        // {1} -> {1}: one entry; with exclude_shared none, by the sets
        r = setpair_record(D, 4, id + 1, id + 1, 1, id + 1, id + 1, 1, false);
        CHECK(r.pair_sum == 0.0 && r.nearest_sum == 0.0);
        float E[16];
        std::fill(E, E + 16, inf);
        r = setpair_record(E, 4, id + 1, id + 1, 1, id + 1, id + 1, 1, false);
        CHECK(r.pair_sum == inf && r.nearest_sum == inf);
        r = setpair_record(E, 4, id + 1, id + 1, 1, id + 1, id + 1, 1, true);
        CHECK(r.pair_sum == 0.0 && r.nearest_sum == 0.0);
        // {0, 1, 2} -> {1} with exclude_shared: element 1 adds +0.0, the others one entry each
        float F[16];
        for (int i = 0; i < 16; i++) F[i] = (float)(i + 1);
        r = setpair_record(F, 4, id, id, 3, id + 1, id + 1, 1, true);
        CHECK(r.pair_sum == 2.0 + 10.0 && r.nearest_sum == 2.0 + 10.0);
        // an empty side: zeros
        r = setpair_record(F, 4, id, id, 0, id, id, 3, false);
        CHECK(r.pair_sum == 0.0 && r.nearest_sum == 0.0);
        r = setpair_record(F, 4, id, id, 3, id, id, 0, false);
        CHECK(r.pair_sum == 0.0 && r.nearest_sum == 0.0 && !std::signbit(r.pair_sum));
    }
    // arguments, in the stated order: each call breaks its check and the next one, and the message is the first's
    {
        Case good;
        good.n = 40;
        for (int k : {3, 7, 40, 1}) add_set(good, k);      // 6 pairs
        std::string err;
        SetpairPlan P;
        CHECK(plan_of(good, 0, 6, 1, 5, 0, P, err) == ST_OK);
        Case c = good;
        c.n = 2;
        CHECK(plan_of(c, 0, 6, 0, -1, 0, P, err) == ST_ERR_ARG && err.find("universe") != std::string::npos);
        c.n = kPermMaxUniverse + 1;
        CHECK(plan_of(c, 0, 6, 0, -1, 0, P, err) == ST_ERR_ARG && err.find("universe") != std::string::npos);
        CHECK(plan_of(good, 0, 6, 0, -1, -1, P, err) == ST_ERR_ARG && err == "permutations < 0");
        CHECK(plan_of(good, 0, 6, 0, 5, -1, P, err, -1) == ST_ERR_ARG && err == "chunk_tasks < 0");
        c = good;
        c.pos[1] = 40;
        CHECK(plan_of(c, 0, 6, 0, 5, 0, P, err, -1) == ST_ERR_ARG && err == "stream < 0");
        CHECK(plan_of(c, -1, 6, 0, 5, 0, P, err) == ST_ERR_ARG && err.find("outside the universe") != std::string::npos);
        c = good;
        std::swap(c.pos[3], c.pos[4]);
        CHECK(plan_of(c, -1, 6, 0, 5, 0, P, err) == ST_ERR_ARG && err.find("increasing") != std::string::npos);
        c = good;
        c.off[2] = c.off[1] - 1;
        CHECK(plan_of(c, -1, 6, 0, 5, 0, P, err) == ST_ERR_ARG && err.find("offsets") != std::string::npos);
        CHECK(setpair_plan(40, nullptr, 3, good.off.data(), 1, -1, 0, 0, 5, 0, 0, P, err) == ST_ERR_ARG && err.find("NULL") != std::string::npos);
        CHECK(setpair_plan(40, good.pos.data(), 3, nullptr, 1, -1, 0, 0, 5, 0, 0, P, err) == ST_ERR_ARG && err.find("NULL") != std::string::npos);
        CHECK(plan_of(good, -1, 9, 0, 5, 0, P, err) == ST_ERR_ARG && err == "a negative triangle range");
        CHECK(plan_of(good, 7, -1, 0, 5, 0, P, err) == ST_ERR_ARG && err == "a negative triangle range");
        CHECK(plan_of(good, 7, 0, 0, 5, 0, P, err) == ST_ERR_ARG && err.find("triangle of 6") != std::string::npos);
        CHECK(plan_of(good, 2, 5, 0, (int64_t)1 << 41, 0, P, err) == ST_ERR_ARG && err.find("triangle of 6") != std::string::npos);
        CHECK(plan_of(good, 6, 0, 0, 5, 0, P, err) == ST_OK && P.chunks.empty());
        CHECK(plan_of(good, 0, 6, 0, ((int64_t)1 << 39) / 6, 0, P, err) == ST_ERR_ARG && err.find("2^40 records") != std::string::npos);
        // a triangle of more than 2^31 pairs, of empty sets
        std::vector<int64_t> many(70001, 0);
        CHECK(setpair_plan(40, nullptr, 0, many.data(), 70000, 0, ((int64_t)1 << 31) + 1, 0, (int64_t)1 << 41, 0, 0, P, err) == ST_ERR_ARG &&
              err.find("2^31 pairs") != std::string::npos);
        CHECK(setpair_plan(40, nullptr, 0, many.data(), 70000, 5, (int64_t)1 << 20, 0, (int64_t)1 << 19, 0, 0, P, err) == ST_ERR_ARG &&
              err.find("2^40 records") != std::string::npos);
        CHECK(setpair_plan(40, nullptr, 0, nullptr, 0, 0, 0, 0, 5, 0, 0, P, err) == ST_OK && P.chunks.empty());
    }
    std::printf("sanitize setpair ok\n");
    return 0;
}
