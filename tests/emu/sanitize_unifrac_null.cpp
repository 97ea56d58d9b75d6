// The host side of Faith's PD and the union sums under the taxa-labels null (suchtree_amd/csrc/unifrac_null_plan.cpp) under
// AddressSanitizer + UBSan (tests/test_unifrac_null_host.py builds this with -fsanitize=address,undefined): the restatement
// against a sum over the distinct relabelled positions with a plain minimum between neighbours, column 0 against
// unifrac_host, chunk cuts that tile every block's tasks once (sets before pairs) and change nothing, the scatter, the
// block bound with the relabelled table counted, and every argument error in its order.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/dispersion_plan.cpp"      // (compiled in here: the program is linked with the two unifrac plans alone)
#include "../../suchtree_amd/csrc/unifrac_null_plan.h"

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

// the union sum of sets a and b under sigma by its definition
static int64_t plain_union(const Case &C, const std::vector<int32_t> &sigma, int64_t a, int64_t b)
{
    std::set<int32_t> u;
    for (int64_t r : {a, b})
        for (int64_t x = C.off[(size_t)r]; x < C.off[(size_t)r + 1]; x++) u.insert(sigma[(size_t)C.pos[(size_t)x]]);
    int64_t sum = 0;
    int32_t prev = -1;
    for (int32_t s : u) {
        sum += C.d_q[(size_t)s];
        if (prev >= 0) sum -= *std::min_element(C.h_q.begin() + prev, C.h_q.begin() + s);
        prev = s;
    }
    return sum;
}

static int plan_of(const Case &C, int64_t begin, int64_t count, int64_t perms, int32_t stream, int64_t chunk, bool pd, bool un, UnifracNullPlan &P,
                   std::string &err)
{
    return unifrac_null_plan(C.n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), (int64_t)C.off.size() - 1, begin, count, perms, stream, chunk,
                             pd, un, P, err);
}

static int check_case(int32_t n, int64_t perms)
{
    Case C;
    C.n = n;
    for (int32_t k = 0; k < n; k++) C.d_q.push_back((int64_t)(rnd() % 2000000) - 1000000);
    for (int32_t k = 0; k + 1 < n; k++) C.h_q.push_back((int64_t)(rnd() % 2000000) - 1000000);
    for (int k : {0, 1, 2, 33, 64, 65})
        if (k <= n) add_random(C, k);
    std::vector<int32_t> all((size_t)n);
    for (int32_t i = 0; i < n; i++) all[(size_t)i] = i;
    add_set(C, all);
    add_set(C, all);      // identical sets
    C.off.push_back((int64_t)C.pos.size());      // an empty set at the end of the table
    const int64_t n_sets = (int64_t)C.off.size() - 1, total = n_sets * (n_sets - 1) / 2, R = perms + 1;
    const uint64_t seed = rnd();
    const int32_t stream = (int32_t)(rnd() % 1000);
    std::string err;
    UnifracNullPlan P;
    CHECK(plan_of(C, 0, total, perms, stream, 0, true, true, P, err) == ST_OK);
    CHECK(P.items == n_sets + total && P.rows == R && P.n_tab == (int64_t)C.pos.size());
    std::vector<int64_t> pd((size_t)(n_sets * R), -1), un((size_t)(total * R), -1);
    unifrac_null_host(C.d_q.data(), C.h_q.data(), P, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), seed, stream, pd.data(), un.data());
    std::vector<int32_t> sigma((size_t)n);
    for (int64_t p = 0; p < R; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        for (int64_t r = 0; r < n_sets; r++) CHECK(pd[(size_t)(r * R + p)] == plain_union(C, sigma, r, r));
        int64_t k = 0;
        for (int64_t i = 0; i < n_sets; i++)
            for (int64_t j = 0; j < i; j++, k++) CHECK(un[(size_t)(k * R + p)] == plain_union(C, sigma, j, i));
    }
    // column 0 is the call without a null
    {
        UnifracPlan U;
        CHECK(unifrac_plan(n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), n_sets, 0, total, 0, true, true, U, err) == ST_OK);
        std::vector<int64_t> pd0((size_t)n_sets), un0((size_t)total);
        unifrac_host(C.d_q.data(), C.h_q.data(), U, C.pos.data(), C.off.data(), pd0.data(), un0.data());
        for (int64_t r = 0; r < n_sets; r++) CHECK(pd0[(size_t)r] == pd[(size_t)(r * R)]);
        for (int64_t k = 0; k < total; k++) CHECK(un0[(size_t)k] == un[(size_t)(k * R)]);
    }
    // cuts: every block's tasks once and in order, at most chunk_tasks a chunk and permutations a block; the scatter puts
    // task t of a block where the restatement put it; a range, a cut and a missing output change nothing
    for (int64_t ct : {1, 3, 7, 64, 0}) {
        const int64_t begin = total / 3, count = total - begin - total / 5;
        for (int want = 1; want < 4; want++) {
            const bool w_pd = want & 1, w_un = (want & 2) && count > 0;
            UnifracNullPlan Q;
            CHECK(plan_of(C, begin, count, perms, stream, ct, w_pd, (want & 2) != 0, Q, err) == ST_OK);
            CHECK(Q.want_pd == w_pd && Q.want_union == w_un && Q.items == (w_un ? n_sets + count : n_sets));
            CHECK(Q.perm_block >= 1 && Q.perm_block <= R && (ct == 0 || Q.perm_block <= ct));
            std::vector<int64_t> pd2((size_t)(n_sets * R), -1), un2((size_t)std::max<int64_t>(count * R, 1), -1);
            int64_t p_next = 0, t_next = 0, np_last = 0;
            for (const DispersionChunk &c : Q.chunks) {
                CHECK(c.n_tasks >= 1 && c.n_tasks <= Q.max_chunk_tasks && (ct == 0 || c.n_tasks <= ct));
                if (np_last > 0 && t_next == Q.items * np_last && c.p_begin != p_next) {      // the block before is complete
                    p_next += np_last;
                    t_next = 0;
                }
                np_last = c.n_perms;
                CHECK(c.p_begin == p_next && c.task_begin == t_next && c.n_perms == std::min(Q.perm_block, R - p_next));
                t_next += c.n_tasks;
                CHECK(t_next <= Q.items * c.n_perms);
                std::vector<int64_t> res((size_t)c.n_tasks);
                for (int64_t j = 0; j < c.n_tasks; j++) {
                    const int64_t t = c.task_begin + j, item = t / c.n_perms, p = c.p_begin + t % c.n_perms;
                    res[(size_t)j] = item < n_sets ? pd[(size_t)(item * R + p)] : un[(size_t)((begin + item - n_sets) * R + p)];
                }
                unifrac_null_scatter(Q, c, res.data(), w_pd ? pd2.data() : nullptr, w_un ? un2.data() : nullptr);
            }
            CHECK(Q.chunks.empty() || (p_next + Q.chunks.back().n_perms == R && t_next == Q.items * Q.chunks.back().n_perms));
            if (w_pd) CHECK(pd2 == pd);
            for (int64_t t = 0; t < count * R && w_un; t++) CHECK(un2[(size_t)t] == un[(size_t)(begin * R + t)]);
            std::fill(pd2.begin(), pd2.end(), -1);
            std::fill(un2.begin(), un2.end(), -1);
            unifrac_null_host(C.d_q.data(), C.h_q.data(), Q, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), seed, stream,
                              w_pd ? pd2.data() : nullptr, w_un ? un2.data() : nullptr);
            if (w_pd) CHECK(pd2 == pd);
            for (int64_t t = 0; t < count * R && w_un; t++) CHECK(un2[(size_t)t] == un[(size_t)(begin * R + t)]);
        }
        UnifracNullPlan Q;
        CHECK(plan_of(C, begin, count, perms, stream, ct, false, false, Q, err) == ST_OK && Q.chunks.empty() && Q.items == 0);
    }
    return 0;
}

int main()
{
    for (int32_t n : {3, 4, 64, 65, 300})
        for (int64_t perms : {0, 1, 5, 6})
            if (check_case(n, perms)) return 1;
    // the block bound counts the relabelled table: 16384 leaves, sets of 16384 positions in all -> half the permutations
    {
        Case C;
        C.n = kPermMaxUniverse;
        std::vector<int32_t> all((size_t)C.n);
        for (int32_t i = 0; i < C.n; i++) all[(size_t)i] = i;
        add_set(C, std::vector<int32_t>(all.begin(), all.begin() + C.n / 2));
        add_set(C, std::vector<int32_t>(all.begin() + C.n / 2, all.end()));
        std::string err;
        UnifracNullPlan A, B;
        CHECK(plan_of(C, 0, 1, 9999, 0, 0, true, false, A, err) == ST_OK && A.n_tab == 0);
        CHECK(plan_of(C, 0, 1, 9999, 0, 0, true, true, B, err) == ST_OK && B.n_tab == C.n);
        CHECK(A.perm_block == kDispersionSigmaBytes / (2 * (int64_t)C.n) && B.perm_block == A.perm_block / 2);
    }
    // arguments, in the order of the contract
    {
        Case good;
        good.n = 40;
        for (int k : {3, 7, 40, 1}) add_random(good, k);
        std::string err;
        UnifracNullPlan P;
        CHECK(plan_of(good, 0, 6, 5, 0, 0, true, true, P, err) == ST_OK);
        CHECK(plan_of(good, 6, 0, 5, 0, 0, true, true, P, err) == ST_OK && !P.want_union && P.items == 4);      // an empty range at the end
        CHECK(plan_of(good, 0, 7, 5, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("triangle") != std::string::npos);
        CHECK(plan_of(good, 7, 0, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, -1, 2, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, 0, -1, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(plan_of(good, 0, 6, -1, 0, 0, true, true, P, err) == ST_ERR_ARG && err == "permutations < 0");
        CHECK(plan_of(good, 0, 6, 5, -1, 0, true, true, P, err) == ST_ERR_ARG && err == "stream < 0");
        CHECK(plan_of(good, 0, 6, 5, 0, -1, true, true, P, err) == ST_ERR_ARG && err == "chunk_tasks < 0");
        CHECK(plan_of(good, 0, 6, ((int64_t)1 << 40) / 4, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("2^40") != std::string::npos);
        Case c = good;
        c.n = 2;
        CHECK(plan_of(c, 0, 6, 5, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("universe") != std::string::npos);
        c.n = kPermMaxUniverse + 1;
        CHECK(plan_of(c, 0, 6, 5, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("universe") != std::string::npos);
        // the order: the universe before permutations before the set table before the range
        c = good;
        c.n = 2;
        c.pos[1] = 40;
        CHECK(plan_of(c, 0, 7, -1, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("universe of 2") != std::string::npos);
        c.n = 40;
        CHECK(plan_of(c, 0, 7, -1, 0, 0, true, true, P, err) == ST_ERR_ARG && err == "permutations < 0");
        CHECK(plan_of(c, 0, 7, 5, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("outside the universe") != std::string::npos);
        c = good;
        std::swap(c.pos[3], c.pos[4]);
        CHECK(plan_of(c, 0, 7, 5, 0, 0, true, true, P, err) == ST_ERR_ARG && err.find("increasing") != std::string::npos);
        c = good;
        c.off[2] = c.off[1] - 1;
        CHECK(plan_of(c, 0, 6, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        c = good;
        c.off.back() += 1;
        CHECK(plan_of(c, 0, 6, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(unifrac_null_plan(40, nullptr, 3, good.off.data(), 1, 0, 0, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);      // NULL arrays
        CHECK(unifrac_null_plan(40, good.pos.data(), 3, nullptr, 1, 0, 0, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(unifrac_null_plan(40, nullptr, 0, nullptr, -1, 0, 0, 5, 0, 0, true, true, P, err) == ST_ERR_ARG);
        CHECK(unifrac_null_plan(40, nullptr, 0, nullptr, 0, 0, 0, 5, 0, 0, true, true, P, err) == ST_OK && P.chunks.empty());
    }
    std::printf("sanitize unifrac null ok\n");
    return 0;
}
