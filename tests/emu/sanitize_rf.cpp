// The host side of the tree-set comparison (suchtree_amd/csrc/rf_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_rf_host.py builds this with -fsanitize=address,undefined): the restatement of Day's method -- the scatter,
// the block extrema, the sparse table, the sorted keys -- against the definition of include/suchtree_hip.h written out
// with sets of positions, over seeded random laminar families at the edges of the blocks of 64 positions and across
// several table levels, both modes, triangle ranges and explicit tasks with alignments, with and without counts, and
// every argument error in the stated order.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/rf_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 3333;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

static std::vector<int32_t> permutation(int32_t m)
{
    std::vector<int32_t> p((size_t)m);
    for (int32_t k = 0; k < m; k++) p[(size_t)k] = k;
    for (int32_t k = m - 1; k > 0; k--) std::swap(p[(size_t)k], p[(size_t)(rnd() % (uint64_t)(k + 1))]);
    return p;
}

// the ranges of a random tree over positions [0, m): a range of two or more positions is split at a random point; the
// ranges the mode admits are listed (unrooted: [k, m) goes where [0, k) is listed); some nodes are skipped (polytomies)
static void family(int32_t m, bool unrooted, std::vector<int32_t> &lo, std::vector<int32_t> &hi)
{
    std::vector<std::pair<int32_t, int32_t>> stack{{0, m}};
    std::vector<char> prefix((size_t)m + 1, 0);
    std::vector<std::pair<int32_t, int32_t>> all;
    while (!stack.empty()) {
        const auto [l, h] = stack.back();
        stack.pop_back();
        if (h - l < 2) continue;
        const int32_t cut = l + 1 + (int32_t)(rnd() % (uint64_t)(h - l - 1));
        stack.push_back({l, cut});
        stack.push_back({cut, h});
        if (h - l <= (unrooted ? m - 2 : m - 1) && rnd() % 8 != 0) all.push_back({l, h});
    }
    for (const auto &r : all)
        if (r.first == 0) prefix[(size_t)r.second] = 1;
    for (const auto &r : all) {
        if (unrooted && r.second == m && prefix[(size_t)r.first]) continue;
        lo.push_back(r.first);
        hi.push_back(r.second);
    }
}

struct Case {
    int32_t m, n_trees;
    bool unrooted;
    std::vector<int32_t> where, lo, hi, align;
    std::vector<int64_t> off;
    int32_t n_align;
};

static Case make_case(int32_t m, int32_t n_trees, bool unrooted, int32_t n_align)
{
    Case c{m, n_trees, unrooted, {}, {}, {}, {}, {0}, n_align};
    for (int32_t t = 0; t < n_trees; t++) {
        const std::vector<int32_t> w = t == 1 ? std::vector<int32_t>(c.where.begin(), c.where.begin() + m) : permutation(m);
        c.where.insert(c.where.end(), w.begin(), w.end());
        if (t == 1) {      // an identical copy of tree 0
            const size_t n = c.lo.size();
            for (size_t r = 0; r < n; r++) {
                c.lo.push_back(c.lo[r]);
                c.hi.push_back(c.hi[r]);
            }
        } else if (t != 2) {      // (tree 2 is a star: no range)
            family(m, unrooted, c.lo, c.hi);
        }
        c.off.push_back((int64_t)c.lo.size());
    }
    for (int32_t r = 0; r < n_align; r++) {
        const std::vector<int32_t> a = permutation(m);
        c.align.insert(c.align.end(), a.begin(), a.end());
    }
    return c;
}

// the definition: Q_b as a sorted list of positions against every range of tree i, and its complement when unrooted
static int32_t naive(const Case &c, int32_t i, int32_t j, int32_t p, std::vector<int64_t> *count)
{
    const int32_t m = c.m, *wi = &c.where[(size_t)i * (size_t)m], *wj = &c.where[(size_t)j * (size_t)m];
    const int32_t *a = p >= 0 ? &c.align[(size_t)p * (size_t)m] : nullptr;
    int32_t shared = 0;
    for (int64_t b = c.off[(size_t)j]; b < c.off[(size_t)j + 1]; b++) {
        std::vector<char> in((size_t)m, 0);
        for (int32_t k = 0; k < m; k++) {
            const int32_t y = wj[a ? a[k] : k];
            if (c.lo[(size_t)b] <= y && y < c.hi[(size_t)b]) in[(size_t)wi[k]] = 1;
        }
        for (int64_t r = c.off[(size_t)i]; r < c.off[(size_t)i + 1]; r++) {
            bool same = true, other = true;
            for (int32_t x = 0; x < m; x++) {
                const bool inside = c.lo[(size_t)r] <= x && x < c.hi[(size_t)r];
                same = same && inside == (in[(size_t)x] != 0);
                other = other && inside != (in[(size_t)x] != 0);
            }
            if (same || (c.unrooted && other)) {
                shared++;
                if (count) {
                    (*count)[(size_t)b]++;
                    (*count)[(size_t)r]++;
                }
                break;
            }
        }
    }
    return shared;
}

static int check_case(const Case &c)
{
    std::string err;
    RfPlan P;
    const int64_t total = (int64_t)c.n_trees * (c.n_trees - 1) / 2;
    std::vector<int32_t> out((size_t)total, -1);
    std::vector<int64_t> count((size_t)c.off.back(), -1), want_count((size_t)c.off.back(), 0);
    const int32_t *align = c.n_align ? c.align.data() : nullptr;
    CHECK(rf_plan(c.m, c.n_trees, c.where.data(), c.off.data(), c.lo.data(), c.hi.data(), c.unrooted, align, c.n_align, nullptr, nullptr, nullptr, total, 0, 0,
                  out.data(), P, err) == ST_OK);
    CHECK(P.triangle && P.n_clades == c.off.back() && std::is_sorted(P.key.begin() + P.off[0], P.key.begin() + P.off[1]));
    rf_host(P, nullptr, nullptr, nullptr, out.data(), count.data());
    for (int64_t k = 0; k < total; k++) {
        int64_t i, j;
        unifrac_pair(k, i, j);
        CHECK(out[(size_t)k] == naive(c, (int32_t)i, (int32_t)j, -1, &want_count));
    }
    CHECK(count == want_count);
    CHECK(out[0] == (int32_t)(c.off[1] - c.off[0]));      // (tree 1 is tree 0)
    // a range of the triangle, without counts
    if (total > 3) {
        std::vector<int32_t> part((size_t)total - 3, -1);
        CHECK(rf_plan(c.m, c.n_trees, c.where.data(), c.off.data(), c.lo.data(), c.hi.data(), c.unrooted, align, c.n_align, nullptr, nullptr, nullptr,
                      total - 3, 2, 5, part.data(), P, err) == ST_OK);
        rf_host(P, nullptr, nullptr, nullptr, part.data(), nullptr);
        CHECK(std::equal(part.begin(), part.end(), out.begin() + 2) && P.chunk == std::min<int64_t>(5, total - 3));
    }
    // explicit tasks with alignments, both directions under the identity
    const int64_t n_tasks = 40;
    std::vector<int32_t> ti, tj, tp, got((size_t)n_tasks, -1);
    for (int64_t t = 0; t < n_tasks; t++) {
        ti.push_back((int32_t)(rnd() % (uint64_t)c.n_trees));
        tj.push_back((int32_t)(rnd() % (uint64_t)c.n_trees));
        tp.push_back((int32_t)(rnd() % (uint64_t)(c.n_align + 1)) - 1);
    }
    CHECK(rf_plan(c.m, c.n_trees, c.where.data(), c.off.data(), c.lo.data(), c.hi.data(), c.unrooted, align, c.n_align, ti.data(), tj.data(), tp.data(), n_tasks,
                  0, 7, got.data(), P, err) == ST_OK);
    std::fill(want_count.begin(), want_count.end(), 0);
    rf_host(P, ti.data(), tj.data(), tp.data(), got.data(), count.data());
    for (int64_t t = 0; t < n_tasks; t++) CHECK(got[(size_t)t] == naive(c, ti[(size_t)t], tj[(size_t)t], tp[(size_t)t], &want_count));
    CHECK(count == want_count);
    std::vector<int32_t> back((size_t)n_tasks, -1);
    CHECK(rf_plan(c.m, c.n_trees, c.where.data(), c.off.data(), c.lo.data(), c.hi.data(), c.unrooted, nullptr, 0, tj.data(), ti.data(), nullptr, n_tasks, 0, 0,
                  back.data(), P, err) == ST_OK);
    rf_host(P, tj.data(), ti.data(), nullptr, back.data(), nullptr);
    for (int64_t t = 0; t < n_tasks; t++) CHECK(back[(size_t)t] == naive(c, ti[(size_t)t], tj[(size_t)t], -1, nullptr));
    return 0;
}

int main()
{
    for (int32_t m : {4, 5, 63, 64, 65, 128, 129, 200, 257})
        for (bool unrooted : {false, true})
            if (check_case(make_case(m, 5, unrooted, 3))) return 1;
    {      // the layout at its edges
        CHECK(rf_blocks(4) == 1 && rf_blocks(64) == 1 && rf_blocks(65) == 2 && rf_blocks(16384) == 256);
        CHECK(rf_levels(1) == 1 && rf_levels(2) == 2 && rf_levels(3) == 2 && rf_levels(129) == 8 && rf_levels(256) == 9);
        CHECK(rf_stride(1) == 8 && rf_stride(129) == 136 && rf_lds_bytes(16384) == 42000 && rf_lds_bytes(4) == 16 + 32 + 16);
        CHECK(rf_canonical(0, 3, 9, true) == rf_key(3, 9) && rf_canonical(0, 3, 9, false) == rf_key(0, 3) && rf_canonical(2, 9, 9, true) == rf_key(2, 9));
        const uint32_t keys[5] = {3, 5, 5, 9, 12};
        CHECK(rf_find(keys, 5, 5) == 1 && rf_find(keys, 5, 3) == 0 && rf_find(keys, 5, 12) == 4 && rf_find(keys, 5, 4) == -1 && rf_find(keys, 0, 4) == -1);
    }
    {      // the cap: a caterpillar against itself reversed, every range size once
        const int32_t m = kRfMaxLeaves;
        Case c{m, 2, true, {}, {}, {}, {}, {0}, 0};
        for (int32_t k = 0; k < m; k++) c.where.push_back(k);
        for (int32_t k = 0; k < m; k++) c.where.push_back(m - 1 - k);
        for (int32_t t = 0; t < 2; t++) {
            for (int32_t s = 2; s <= m - 2; s++) {
                c.lo.push_back(0);
                c.hi.push_back(s);
            }
            c.off.push_back((int64_t)c.lo.size());
        }
        std::string err;
        RfPlan P;
        int32_t out = -1;
        std::vector<int64_t> count((size_t)c.off.back(), -1);
        CHECK(rf_plan(m, 2, c.where.data(), c.off.data(), c.lo.data(), c.hi.data(), true, nullptr, 0, nullptr, nullptr, nullptr, 1, 0, 0, &out, P, err) == ST_OK);
        rf_host(P, nullptr, nullptr, nullptr, &out, count.data());
        // tree 1's prefix [0, s) is tree 0's suffix [m - s, m): the bipartition of tree 0's prefix of m - s
        CHECK(out == m - 3 && std::all_of(count.begin(), count.end(), [](int64_t v) { return v == 1; }));
    }
    {      // the argument checks, in the stated order
        std::string err;
        RfPlan P;
        std::vector<int32_t> where = {0, 1, 2, 3, 4, 4, 3, 2, 1, 0}, lo = {0, 2, 1}, hi = {2, 5, 3}, align = {0, 1, 2, 3, 4}, out(1), ti = {0}, tj = {1}, tp = {0};
        std::vector<int64_t> off = {0, 2, 3};
        auto plan = [&](int32_t m, int32_t n_trees, const int32_t *w, const int64_t *o, const int32_t *l, const int32_t *h, const int32_t *al, int32_t n_align,
                        const int32_t *i, const int32_t *j, const int32_t *p, int64_t n_tasks, int64_t begin, int64_t chunk, const int32_t *res) {
            return rf_plan(m, n_trees, w, o, l, h, true, al, n_align, i, j, p, n_tasks, begin, chunk, res, P, err);
        };
        const int32_t *W = where.data(), *L = lo.data(), *H = hi.data(), *A = align.data(), *N = nullptr;
        const int64_t *O = off.data();
        CHECK(plan(3, -1, N, nullptr, N, N, N, -1, N, N, N, -1, -1, -1, N) == ST_ERR_ARG && err.find("a list of 3 leaves") == 0);
        CHECK(plan(kRfMaxLeaves + 1, 2, W, O, L, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err.find("a list of 16385 leaves") == 0);
        CHECK(plan(5, -1, N, nullptr, N, N, N, 0, N, N, N, 0, -1, -1, N) == ST_ERR_ARG && err == "negative size");
        CHECK(plan(5, 2, N, nullptr, N, N, N, 0, N, N, N, 0, -1, -1, N) == ST_ERR_ARG && err == "begin < 0");
        CHECK(plan(5, 2, N, nullptr, N, N, N, 0, N, N, N, 0, 0, -1, N) == ST_ERR_ARG && err == "chunk_tasks < 0");
        CHECK(plan(5, 2, N, O, L, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err == "where or clade_offsets is NULL");
        CHECK(plan(5, 2, W, O, L, H, N, 1, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err == "align is NULL");
        off[1] = 4;
        CHECK(plan(5, 2, W, O, L, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err.find("clade_offsets[2] = 3") == 0);
        off[1] = 2;
        CHECK(plan(5, 2, W, O, N, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err == "lo or hi is NULL");
        where[7] = 4;
        CHECK(plan(5, 2, W, O, L, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err.find("where[1][2] = 4") == 0);
        where[7] = 2;
        hi[2] = 6;
        CHECK(plan(5, 2, W, O, L, H, N, 0, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err == "tree 1, range 0: [1, 6) of 5 positions");
        hi[2] = 3;
        align[4] = 5;
        CHECK(plan(5, 2, W, O, L, H, A, 1, N, N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err.find("align[0][4] = 5") == 0);
        align[4] = 4;
        CHECK(plan(5, 2, W, O, L, H, A, 1, N, N, N, 2, 0, 0, out.data()) == ST_ERR_ARG && err == "pairs [0, +2) of a triangle of 1");
        CHECK(plan(5, 2, W, O, L, H, A, 1, N, N, tp.data(), 1, 0, 0, out.data()) == ST_ERR_ARG && err == "task_p without task_i and task_j");
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), N, N, 1, 0, 0, out.data()) == ST_ERR_ARG && err == "task_i or task_j is NULL");
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), tj.data(), N, 1, 1, 0, out.data()) == ST_ERR_ARG && err == "begin = 1 with explicit tasks");
        tj[0] = 2;
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), tj.data(), N, 1, 0, 0, out.data()) == ST_ERR_BOUNDS && err == "task 0: trees (0, 2) of 2");
        tj[0] = 1;
        tp[0] = 1;
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), tj.data(), tp.data(), 1, 0, 0, out.data()) == ST_ERR_BOUNDS && err == "task 0: alignment 1 of 1");
        tp[0] = 0;
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), tj.data(), tp.data(), 1, 0, 0, N) == ST_ERR_ARG && err == "out_shared is NULL");
        CHECK(plan(5, 2, W, O, L, H, A, 1, ti.data(), tj.data(), tp.data(), 1, 0, 0, out.data()) == ST_OK && !P.triangle && P.chunk == 1);
        CHECK(plan(5, 2, W, O, L, H, A, 1, N, N, N, 0, 1, 0, N) == ST_OK && P.n_tasks == 0);
        rf_host(P, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    std::printf("sanitize rf ok\n");
    return 0;
}
