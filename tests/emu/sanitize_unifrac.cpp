// The host side of Faith's PD and the union sums behind UniFrac (suchtree_amd/csrc/unifrac_plan.cpp) under
// AddressSanitizer + UBSan (tests/test_unifrac_host.py builds this with -fsanitize=address,undefined): the range-minimum
// table at n = 1, 2, 3 and 2^k +- 1 against a plain minimum, the pair order, chunk cuts that tile the tasks once, the merge
// and the successor form on their edges against a sum over distinct positions, the quantiser, and every argument error.
// Malformed set tables go to dispersion_plan as well: the two plans share that check (plan_checks.h) and word it alike.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/dispersion_plan.cpp"      // (compiled in here: the program is linked with unifrac_plan.cpp alone)
#include "../../suchtree_amd/csrc/unifrac_plan.h"

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
    std::vector<int64_t> d_q, h_q;
    std::vector<int32_t> pos;
    std::vector<int64_t> off{0};
};

static void add_set(Case &C, std::vector<int32_t> s)
{
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    C.pos.insert(C.pos.end(), s.begin(), s.end());
    C.off.push_back((int64_t)C.pos.size());
}

static void add_random(Case &C, int k)
{
    std::vector<int32_t> all((size_t)C.n);
    for (int32_t i = 0; i < C.n; i++) all[(size_t)i] = i;
    for (int i = 0; i < k; i++) std::swap(all[(size_t)i], all[(size_t)i + rnd() % (uint64_t)(C.n - i)]);
    add_set(C, std::vector<int32_t>(all.begin(), all.begin() + k));
}

static int64_t plain_min(const Case &C, int32_t x, int32_t y) { return *std::min_element(C.h_q.begin() + x, C.h_q.begin() + y); }

// the union sum by its definition: the distinct positions in order, a plain minimum between neighbours
static int64_t plain_union(const Case &C, int64_t a, int64_t b)
{
    std::set<int32_t> u(C.pos.begin() + C.off[(size_t)a], C.pos.begin() + C.off[(size_t)a + 1]);
    u.insert(C.pos.begin() + C.off[(size_t)b], C.pos.begin() + C.off[(size_t)b + 1]);
    int64_t sum = 0;
    int32_t prev = -1;
    for (int32_t s : u) {
        sum += C.d_q[(size_t)s];
        if (prev >= 0) sum -= plain_min(C, prev, s);
        prev = s;
    }
    return sum;
}

static int plan_of(const Case &C, int64_t begin, int64_t count, int64_t chunk, bool pd, bool un, UnifracPlan &P, std::string &err)
{
    return unifrac_plan(C.n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), (int64_t)C.off.size() - 1, begin, count, chunk, pd, un, P, err);
}

static int check_case(int32_t n)
{
    Case C;
    C.n = n;
    for (int32_t k = 0; k < n; k++) C.d_q.push_back((int64_t)(rnd() % 2000000) - 1000000);
    for (int32_t k = 0; k + 1 < n; k++) C.h_q.push_back((int64_t)(rnd() % 2000000) - 1000000);
    const int64_t m = n - 1;
    const int levels = unifrac_levels(m);
    CHECK(m == 0 ? levels == 0 : (((int64_t)1 << (levels - 1)) <= m && m < ((int64_t)1 << levels)));
    std::vector<int64_t> M((size_t)(levels * m));
    unifrac_table(C.h_q.data(), m, levels, M.data());
    // every query of length 1, 2^l - 1, 2^l, 2^l + 1 and the whole range, from both ends and from random starts
    for (int64_t len = 1; len <= m; len++) {
        bool edge = len == m;
        for (int l = 0; l < 21; l++) edge = edge || len == ((int64_t)1 << l) - 1 || len == ((int64_t)1 << l) || len == ((int64_t)1 << l) + 1;
        if (!edge && rnd() % 16) continue;
        for (int32_t x : {(int32_t)0, (int32_t)(m - len), (int32_t)(rnd() % (uint64_t)(m - len + 1))})
            CHECK(unifrac_rmq(M.data(), m, x, (int32_t)(x + len)) == plain_min(C, x, (int32_t)(x + len)));
    }
    for (int k : {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 257})
        if (k <= n) add_random(C, k);
    std::vector<int32_t> all((size_t)n);
    for (int32_t i = 0; i < n; i++) all[(size_t)i] = i;
    add_set(C, all);                                                                    // the universe ...
    add_set(C, all);                                                                    // ... twice: identical sets
    add_set(C, std::vector<int32_t>(all.begin(), all.begin() + n / 2));                 // nested
    add_set(C, std::vector<int32_t>(all.begin() + n / 2, all.end()));                   // disjoint from it, adjacent to it
    add_set(C, {0, n - 1});
    add_set(C, {0});
    add_set(C, {n - 1});
    const int64_t n_sets = (int64_t)C.off.size() - 1, total = n_sets * (n_sets - 1) / 2;
    std::string err;
    UnifracPlan P;
    CHECK(plan_of(C, 0, total, 0, true, true, P, err) == ST_OK);
    CHECK(P.n == n && P.m == m && P.levels == levels && P.n_sets == n_sets);
    std::vector<int64_t> pd((size_t)n_sets, -1), un((size_t)total, -1);
    unifrac_host(C.d_q.data(), C.h_q.data(), P, C.pos.data(), C.off.data(), pd.data(), un.data());
    for (int64_t r = 0; r < n_sets; r++) CHECK(pd[(size_t)r] == plain_union(C, r, r));
    int64_t k = 0;
    for (int64_t i = 0; i < n_sets; i++)
        for (int64_t j = 0; j < i; j++, k++) {
            int64_t pi, pj;
            unifrac_pair(k, pi, pj);
            CHECK(pi == i && pj == j);
            const int64_t want = plain_union(C, j, i);
            CHECK(un[(size_t)k] == want);
            const int32_t *A = C.pos.data() + C.off[(size_t)j], *B = C.pos.data() + C.off[(size_t)i];
            const int64_t na = C.off[(size_t)j + 1] - C.off[(size_t)j], nb = C.off[(size_t)i + 1] - C.off[(size_t)i];
            CHECK(unifrac_union_successor(C.d_q.data(), M.data(), m, A, na, B, nb) == want);
            CHECK(unifrac_union_successor(C.d_q.data(), M.data(), m, B, nb, A, na) == want);
            CHECK(unifrac_union(C.d_q.data(), M.data(), m, B, nb, A, na) == want);
        }
    // chunk cuts tile the tasks once, in order; a range and a cut change nothing
    for (int64_t cb : {1, 2, 7, 64, 0}) {
        const int64_t begin = total / 3, count = total - begin - total / 5;
        UnifracPlan Q;
        CHECK(plan_of(C, begin, count, cb, true, true, Q, err) == ST_OK);
        int64_t next_pd = 0, next_un = 0;
        for (const UnifracChunk &c : Q.chunks) {
            CHECK(c.count >= 1 && c.count <= Q.max_chunk && (cb == 0 || c.count <= cb));
            if (c.kind == kUnifracPD) {
                CHECK(next_un == 0 && c.begin == next_pd && c.out_at == next_pd);
                next_pd += c.count;
            } else {
                CHECK(c.kind == kUnifracPairs && next_pd == n_sets && c.begin == begin + next_un && c.out_at == next_un);
                next_un += c.count;
            }
        }
        CHECK(next_pd == n_sets && next_un == count);
        std::vector<int64_t> pd2((size_t)n_sets, -1), un2((size_t)std::max<int64_t>(count, 1), -1);
        unifrac_host(C.d_q.data(), C.h_q.data(), Q, C.pos.data(), C.off.data(), pd2.data(), un2.data());
        CHECK(pd2 == pd);
        for (int64_t t = 0; t < count; t++) CHECK(un2[(size_t)t] == un[(size_t)(begin + t)]);
        CHECK(plan_of(C, begin, count, cb, false, true, Q, err) == ST_OK && (Q.chunks.empty() || Q.chunks[0].kind == kUnifracPairs));
        CHECK(plan_of(C, begin, count, cb, true, false, Q, err) == ST_OK && Q.chunks.back().kind == kUnifracPD);
        CHECK(plan_of(C, begin, count, cb, false, false, Q, err) == ST_OK && Q.chunks.empty());
    }
    return 0;
}

int main()
{
    for (int32_t n : {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025})
        if (check_case(n)) return 1;
    // the pair order far out, and the integer root at its edges
    for (uint64_t r : {0ull, 1ull, 2ull, 3ull, 4ull, 15ull, 16ull, 17ull, (1ull << 32) - 1, 1ull << 32, (1ull << 62) - 1, 1ull << 62, (1ull << 63) - 1}) {
        const uint64_t s = unifrac_isqrt(r);
        CHECK(s * s <= r && (s + 1 > 3037000499ull || (s + 1) * (s + 1) > r));
    }
    for (int64_t i : {(int64_t)1, (int64_t)2, (int64_t)65535, (int64_t)65536, (int64_t)1 << 20, ((int64_t)1 << 30) - 1})
        for (int64_t j : {(int64_t)0, i / 2, i - 1}) {
            int64_t pi, pj;
            unifrac_pair(i * (i - 1) / 2 + j, pi, pj);
            CHECK(pi == i && pj == j);
        }
    // the quantiser
    {
        std::string err;
        int32_t used = -7;
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (float top : {1.0f, 1.9999999f, 3.0e38f, 1.0e-45f, 0.75f}) {
            const float d[3] = {top, -top / 3, 0.0f}, h[2] = {top / 7, -top};
            int64_t dq[3], hq[2];
            CHECK(unifrac_quantise(d, h, 3, -1, dq, hq, &used, err) == ST_OK && used == 39 - std::ilogb(top));
            CHECK(dq[0] >= (int64_t)1 << 39 && dq[0] < kUnifracQLimit && hq[1] == -dq[0] && dq[2] == 0);
            CHECK(unifrac_depth_args(dq, hq, 3, err) == ST_OK);
            CHECK(unifrac_quantise(d, h, 3, -1, nullptr, nullptr, nullptr, err) == ST_OK);
        }
        const float z[2] = {0.0f, -0.0f}, zh[1] = {0.0f};
        int64_t dq[2], hq[1];
        CHECK(unifrac_quantise(z, zh, 2, -1, dq, hq, &used, err) == ST_OK && used == 0 && dq[0] == 0 && dq[1] == 0 && hq[0] == 0);
        CHECK(unifrac_quantise(z, nullptr, 1, -1, dq, nullptr, &used, err) == ST_OK);
        const float one[2] = {1.0f, 0.5f}, two[2] = {2.0f, 0.5f}, bad_a[2] = {1.0f, nan}, bad_b[2] = {inf, 1.0f}, bh[1] = {-inf};
        CHECK(unifrac_quantise(one, zh, 2, 39, dq, hq, &used, err) == ST_OK && used == 39 && dq[0] == (int64_t)1 << 39 && dq[1] == (int64_t)1 << 38);
        CHECK(unifrac_quantise(one, zh, 2, 40, dq, hq, &used, err) == ST_ERR_ARG && !err.empty());
        CHECK(unifrac_quantise(two, zh, 2, 39, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(one, two, 2, 39, dq, hq, &used, err) == ST_ERR_ARG);      // h counts as well
        CHECK(unifrac_quantise(one, zh, 2, 0, dq, hq, &used, err) == ST_OK && dq[0] == 1 && dq[1] == 0);      // 0.5: half to even
        CHECK(unifrac_quantise(one, zh, 2, kUnifracMaxShift, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(z, zh, 2, kUnifracMaxShift, dq, hq, &used, err) == ST_OK && used == kUnifracMaxShift);
        CHECK(unifrac_quantise(one, zh, 2, -2, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(one, zh, 2, kUnifracMaxShift + 1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(bad_a, zh, 2, -1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(bad_b, zh, 2, -1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(one, bh, 2, -1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(one, zh, 0, -1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(nullptr, zh, 2, -1, dq, hq, &used, err) == ST_ERR_ARG);
        CHECK(unifrac_quantise(one, nullptr, 2, -1, dq, hq, &used, err) == ST_ERR_ARG);
        int64_t big[2] = {kUnifracQLimit - 1, -(kUnifracQLimit - 1)}, bigh[1] = {kUnifracQLimit};
        CHECK(unifrac_depth_args(big, hq, 2, err) == ST_OK);
        CHECK(unifrac_depth_args(big, bigh, 2, err) == ST_ERR_ARG);
        big[1] = -kUnifracQLimit;
        CHECK(unifrac_depth_args(big, hq, 2, err) == ST_ERR_ARG);
        CHECK(unifrac_depth_args(nullptr, hq, 2, err) == ST_ERR_ARG && unifrac_depth_args(big, nullptr, 2, err) == ST_ERR_ARG);
    }
    // arguments
    {
        Case good;
        good.n = 40;
        for (int k : {3, 7, 40, 1}) add_random(good, k);
        std::string err;
        UnifracPlan P;
        CHECK(plan_of(good, 0, 6, 0, true, true, P, err) == ST_OK);
        CHECK(plan_of(good, 6, 0, 0, true, true, P, err) == ST_OK);                 // an empty range at the end
        CHECK(plan_of(good, 0, 7, 0, true, true, P, err) == ST_ERR_ARG && !err.empty());      // past the triangle
        CHECK(plan_of(good, 7, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, -1, 2, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, 0, -1, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, 0, 6, -1, true, true, P, err) == ST_ERR_ARG);           // negative chunk_pairs
        Case c = good;
        c.n = 0;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // a universe below 1 ...
        c.n = kUnifracMaxUniverse + 1;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // ... and above the limit
        c.n = kUnifracMaxUniverse;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_OK && P.levels == 20);
        c = good;
        c.pos[1] = 40;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // a position outside the universe
        c.pos[1] = -1;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);
        c = good;
        std::swap(c.pos[3], c.pos[4]);
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG && err.find("increasing") != std::string::npos);
        c = good;
        c.pos[4] = c.pos[3];
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // a duplicate
        c = good;
        c.off[2] = c.off[1] - 1;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // offsets that go back
        c = good;
        c.off.back() += 1;
        CHECK(plan_of(c, 0, 6, 0, true, true, P, err) == ST_ERR_ARG);               // offsets past the positions
        CHECK(unifrac_plan(40, nullptr, 3, good.off.data(), 1, 0, 0, 0, true, true, P, err) == ST_ERR_ARG);      // NULL arrays
        CHECK(unifrac_plan(40, good.pos.data(), 3, nullptr, 1, 0, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(unifrac_plan(40, nullptr, 0, nullptr, -1, 0, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(unifrac_plan(40, nullptr, 0, nullptr, 0, 0, 0, 0, true, true, P, err) == ST_OK && P.chunks.empty());
    }
    // malformed set tables over a universe of 3: both plans refuse each, in the same words
    {
        struct Bad {
            const char *what;
            std::vector<int32_t> pos;
            std::vector<int64_t> off;
            bool null_pos, null_off;
        };
        const Bad table[] = {
            {"a negative offset", {0, 1}, {-1, 2}, false, false},
            {"a decreasing offset", {0, 1}, {0, 2, 1}, false, false},
            {"an offset past n_pos", {0, 1}, {0, 3}, false, false},
            {"a position -1", {-1, 1}, {0, 2}, false, false},
            {"a position equal to n", {0, 3}, {0, 2}, false, false},
            {"a repeated position", {1, 1}, {0, 2}, false, false},
            {"a decreasing position", {2, 1}, {0, 2}, false, false},
            {"NULL sets with n_sets = 1", {0}, {0, 1}, false, true},
            {"NULL set_pos with n_pos = 1", {0}, {0, 1}, true, false},
        };
        for (const Bad &b : table) {
            const int32_t *pos = b.null_pos ? nullptr : b.pos.data();
            const int64_t *off = b.null_off ? nullptr : b.off.data();
            const int64_t n_pos = (int64_t)b.pos.size(), n_sets = (int64_t)b.off.size() - 1;
            std::string err_d, err_u;
            DispersionPlan D;
            UnifracPlan U;
            const int rc_d = dispersion_plan(3, pos, n_pos, off, n_sets, 5, 0, 0, D, err_d);
            const int rc_u = unifrac_plan(3, pos, n_pos, off, n_sets, 0, 0, 0, true, true, U, err_u);
            if (rc_d != ST_ERR_ARG || rc_u != ST_ERR_ARG || err_d.empty() || err_d != err_u) {
                std::printf("FAILED %s: dispersion_plan %d \"%s\", unifrac_plan %d \"%s\"\n", b.what, rc_d, err_d.c_str(), rc_u, err_u.c_str());
                return 1;
            }
        }
    }
    std::printf("sanitize unifrac ok\n");
    return 0;
}
