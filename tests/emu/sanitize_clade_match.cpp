// The host side of the clade matching (suchtree_amd/csrc/clade_match_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_clade_match_host.py builds this with -fsanitize=address,undefined): the range builder on random binary
// trees and on a strict subset of their leaves against leaf sets gathered node by node, the restatement and the windowed
// form against a plain count of shared leaves at m = 4, 5, 63, 64, 65, 128 and 129 in both modes (the word edges of the
// kernel's bitmap, rank(m) included), a tie, no candidates, and every argument error.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/clade_match_plan.h"

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

// a random binary tree of n leaves: ids in join order (leaves first), the root last
static std::vector<int32_t> random_parent(int32_t n)
{
    std::vector<int32_t> parent((size_t)(2 * n - 1), -1), open;
    for (int32_t v = 0; v < n; v++) open.push_back(v);
    for (int32_t v = n; v < 2 * n - 1; v++)
        for (int k = 0; k < 2; k++) {
            const size_t at = (size_t)(rnd() % open.size());
            parent[(size_t)open[at]] = v;
            open[at] = open.back();
            open.pop_back();
            if (k == 1) open.push_back(v);
        }
    return parent;
}

struct Side {
    std::vector<int32_t> order, node, lo, hi;
};

// the listed leaves (as list indices) under every node, gathered leaf by leaf
static std::vector<std::set<int32_t>> leaf_sets(const std::vector<int32_t> &parent, const std::vector<int64_t> &ids)
{
    std::vector<std::set<int32_t>> under(parent.size());
    for (size_t k = 0; k < ids.size(); k++)
        for (int64_t v = ids[k]; v >= 0; v = parent[(size_t)v]) under[(size_t)v].insert((int32_t)k);
    return under;
}

static int check_ranges(const std::vector<int32_t> &parent, const std::vector<int64_t> &ids, bool rooted, Side &S)
{
    const int32_t m = (int32_t)ids.size();
    std::string err;
    int64_t bad = -1;
    CHECK(clade_ranges(parent.data(), (int64_t)parent.size(), ids.data(), m, rooted, S.order, S.node, S.lo, S.hi, &bad, err) == ST_OK);
    CHECK((int32_t)S.order.size() == m);
    std::vector<int32_t> where((size_t)m, -1);      // position of list index k
    for (int32_t p = 0; p < m; p++) {
        CHECK(S.order[(size_t)p] >= 0 && S.order[(size_t)p] < m && where[(size_t)S.order[(size_t)p]] < 0);
        where[(size_t)S.order[(size_t)p]] = p;
    }
    const auto under = leaf_sets(parent, ids);
    // every listed clade is the range of its node's set; the sets are distinct; the sizes are eligible
    std::set<std::set<int32_t>> seen;
    for (size_t r = 0; r < S.node.size(); r++) {
        const std::set<int32_t> &s = under[(size_t)S.node[r]];
        const int32_t size = S.hi[r] - S.lo[r];
        CHECK((int32_t)s.size() == size && size >= 2 && size <= (rooted ? m - 1 : m - 2));
        for (int32_t k : s) CHECK(where[(size_t)k] >= S.lo[r] && where[(size_t)k] < S.hi[r]);
        CHECK(seen.insert(s).second);
    }
    // and every distinct set of an eligible size is listed, but for the one complement of an unrooted list
    std::set<std::set<int32_t>> all;
    for (size_t v = 0; v < parent.size(); v++)
        if ((int32_t)under[v].size() >= 2 && (int32_t)under[v].size() <= (rooted ? m - 1 : m - 2)) all.insert(under[v]);
    size_t dropped = 0;
    for (const auto &s : all)
        if (!seen.count(s)) {
            std::set<int32_t> rest;
            for (int32_t k = 0; k < m; k++)
                if (!s.count(k)) rest.insert(k);
            CHECK(!rooted && seen.count(rest) && s.count(S.order[(size_t)m - 1]));      // ([k, m) went, [0, k) stayed)
            dropped++;
        }
    CHECK(dropped <= 1 && seen.size() + dropped == all.size());
    return 0;
}

static int check_match(const Side &A, const Side &B, int32_t m, bool unrooted)
{
    std::vector<int32_t> where_b((size_t)m), pos_b((size_t)m);
    for (int32_t p = 0; p < m; p++) where_b[(size_t)B.order[(size_t)p]] = p;
    for (int32_t p = 0; p < m; p++) pos_b[(size_t)p] = where_b[(size_t)A.order[(size_t)p]];
    const int32_t n_a = (int32_t)A.node.size(), n_b = (int32_t)B.node.size();
    std::string err;
    CHECK(clade_match_args(m, pos_b.data(), A.lo.data(), A.hi.data(), n_a, B.lo.data(), B.hi.data(), n_b, 0, err) == ST_OK);
    std::vector<int32_t> dist((size_t)n_a + 1, -7), match(dist), inter(dist);
    clade_match_host(m, pos_b.data(), A.lo.data(), A.hi.data(), n_a, B.lo.data(), B.hi.data(), n_b, unrooted, dist.data(), match.data(), inter.data());
    for (int32_t r = 0; r < n_a; r++) {      // a plain count of shared leaves
        int32_t best_d = -1, best_c = -1, best_i = 0;
        for (int32_t c = 0; c < n_b; c++) {
            int32_t i = 0;
            for (int32_t k = A.lo[(size_t)r]; k < A.hi[(size_t)r]; k++) i += pos_b[(size_t)k] >= B.lo[(size_t)c] && pos_b[(size_t)k] < B.hi[(size_t)c];
            const int32_t d = (A.hi[(size_t)r] - A.lo[(size_t)r]) + (B.hi[(size_t)c] - B.lo[(size_t)c]) - 2 * i;
            const int32_t delta = unrooted ? std::min(d, m - d) : d;
            if (best_c < 0 || delta < best_d) {
                best_d = delta;
                best_c = c;
                best_i = i;
            }
        }
        CHECK(dist[(size_t)r] == best_d && match[(size_t)r] == best_c && inter[(size_t)r] == best_i);
    }
    CHECK(dist[(size_t)n_a] == -7);
    for (const bool window : {true, false})
        for (const int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)7}) {
            CladeMatchPlan P;
            clade_match_plan(m, A.lo.data(), A.hi.data(), n_a, B.lo.data(), B.hi.data(), n_b, unrooted, chunk, window, P);
            CHECK(P.chunk >= 1 && (int32_t)P.b_idx.size() == n_b && (int32_t)P.win.size() == 4 * n_a);
            for (int32_t c = 0; c + 1 < n_b; c++) {      // by size, stable
                const int32_t s0 = P.b_hi[(size_t)c] - P.b_lo[(size_t)c], s1 = P.b_hi[(size_t)c + 1] - P.b_lo[(size_t)c + 1];
                CHECK(s0 < s1 || (s0 == s1 && P.b_idx[(size_t)c] < P.b_idx[(size_t)c + 1]));
            }
            for (int32_t r = 0; r < n_a; r++) {
                const int32_t *w = &P.win[(size_t)r * 4];
                CHECK(0 <= w[0] && w[0] <= w[1] && w[1] <= n_b && 0 <= w[2] && w[2] <= w[3] && w[3] <= n_b);
                CHECK(w[2] == w[3] || w[1] < w[2]);
                if (!window) CHECK(w[1] == 0 && w[3] == 0);
            }
            std::vector<int32_t> d2((size_t)n_a + 1, -7), m2(d2), i2(d2);
            clade_match_windowed_host(P, pos_b.data(), A.lo.data(), A.hi.data(), d2.data(), m2.data(), i2.data());
            CHECK(d2 == dist && m2 == match && i2 == inter);
        }
    return 0;
}

int main()
{
    for (const int32_t m : {4, 5, 63, 64, 65, 128, 129})
        for (const bool rooted : {false, true}) {
            const std::vector<int32_t> pa = random_parent(m), pb = random_parent(m);
            std::vector<int64_t> ids_a((size_t)m), ids_b((size_t)m);
            for (int32_t k = 0; k < m; k++) ids_a[(size_t)k] = ids_b[(size_t)k] = k;
            for (int32_t k = m - 1; k > 0; k--) std::swap(ids_b[(size_t)k], ids_b[(size_t)(rnd() % (uint64_t)(k + 1))]);
            Side A, B;
            if (check_ranges(pa, ids_a, rooted, A) || check_ranges(pb, ids_b, rooted, B)) return 1;
            // binary: m - 1 kept nodes; the root's set goes, and unrooted one more: its child of m - 1 leaves or a complement
            CHECK((int32_t)A.node.size() == (rooted ? m - 2 : m - 3) && B.node.size() == A.node.size());
            if (check_match(A, B, m, !rooted) || check_match(A, A, m, !rooted)) return 1;
            // a tree against itself: every row finds itself
            {
                std::vector<int32_t> pos((size_t)m), d((size_t)A.node.size()), mt(d), in(d);
                for (int32_t k = 0; k < m; k++) pos[(size_t)k] = k;
                clade_match_host(m, pos.data(), A.lo.data(), A.hi.data(), (int32_t)A.node.size(), A.lo.data(), A.hi.data(), (int32_t)A.node.size(),
                                 !rooted, d.data(), mt.data(), in.data());
                for (size_t r = 0; r < d.size(); r++) CHECK(d[r] == 0 && mt[r] == (int32_t)r && in[r] == A.hi[r] - A.lo[r]);
            }
            // a strict subset of the leaves: nodes collapse
            if (m >= 63) {
                std::vector<int64_t> sub_a, sub_b;
                for (int32_t k = 0; k < m; k += 1 + (int32_t)(rnd() % 3)) {
                    sub_a.push_back(ids_a[(size_t)k]);
                    sub_b.push_back(ids_b[(size_t)k]);
                }
                Side SA, SB;
                if (check_ranges(pa, sub_a, rooted, SA) || check_ranges(pb, sub_b, rooted, SB)) return 1;
                if (check_match(SA, SB, (int32_t)sub_a.size(), !rooted)) return 1;
            }
        }
    {      // a tie goes to the lower index; no candidates; one candidate list given twice over
        const int32_t m = 8, pos[8] = {0, 1, 2, 3, 4, 5, 6, 7}, a_lo[1] = {2}, a_hi[1] = {4}, b_lo[3] = {4, 1, 2}, b_hi[3] = {6, 3, 5};
        int32_t d = -7, mt = -7, in = -7;
        clade_match_host(m, pos, a_lo, a_hi, 1, b_lo, b_hi, 3, false, &d, &mt, &in);      // {2,3} against {4,5}: 4; {1,2}: 2; {2,3,4}: 1
        CHECK(d == 1 && mt == 2 && in == 2);
        const int32_t t_lo[2] = {1, 3}, t_hi[2] = {3, 5};      // {1,2} and {3,4}: both at 2 from {2,3}
        clade_match_host(m, pos, a_lo, a_hi, 1, t_lo, t_hi, 2, true, &d, &mt, &in);
        CHECK(d == 2 && mt == 0 && in == 1);
        clade_match_host(m, pos, a_lo, a_hi, 1, nullptr, nullptr, 0, true, &d, &mt, &in);
        CHECK(d == -1 && mt == -1 && in == 0);
        CladeMatchPlan P;
        clade_match_plan(m, a_lo, a_hi, 1, nullptr, nullptr, 0, true, 0, true, P);
        clade_match_windowed_host(P, pos, a_lo, a_hi, &d, &mt, &in);
        CHECK(d == -1 && mt == -1 && in == 0);
    }
    {      // argument errors
        std::string err;
        const int32_t pos[4] = {0, 1, 2, 3}, lo[1] = {0}, hi[1] = {2};
        CHECK(clade_match_args(4, pos, lo, hi, 1, lo, hi, 1, 0, err) == ST_OK);
        CHECK(clade_match_args(3, pos, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(kCladeMatchMaxLeaves + 1, pos, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, lo, hi, -1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, lo, hi, 1, lo, hi, 1, -1, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, nullptr, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, nullptr, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, lo, hi, 1, lo, nullptr, 1, 0, err) == ST_ERR_ARG);
        const int32_t twice[4] = {0, 1, 1, 3}, outside[4] = {0, 1, 2, 4}, neg[4] = {0, -1, 2, 3};
        CHECK(clade_match_args(4, twice, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, outside, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, neg, lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        const int32_t empty_hi[1] = {0}, past_hi[1] = {5}, neg_lo[1] = {-1};
        CHECK(clade_match_args(4, pos, lo, empty_hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, lo, hi, 1, lo, past_hi, 1, 0, err) == ST_ERR_ARG);
        CHECK(clade_match_args(4, pos, neg_lo, hi, 1, lo, hi, 1, 0, err) == ST_ERR_ARG);
        // the range builder: a bad parent array, ids outside, no leaf, twice
        const int32_t parent[7] = {4, 4, 5, 5, 6, 6, -1};
        const int64_t ids[4] = {0, 1, 2, 3}, out_ids[4] = {0, 1, 2, 7}, inner[4] = {0, 1, 2, 4}, rep[4] = {0, 1, 2, 2};
        std::vector<int32_t> o, n, l, h;
        int64_t bad = -1;
        CHECK(clade_ranges(parent, 7, ids, 4, false, o, n, l, h, &bad, err) == ST_OK && n.size() == 1 && l[0] == 0 && h[0] == 2);
        CHECK(clade_ranges(parent, 7, ids, 4, true, o, n, l, h, &bad, err) == ST_OK && n.size() == 2);
        CHECK(clade_ranges(parent, 7, out_ids, 4, false, o, n, l, h, &bad, err) == ST_ERR_BOUNDS && bad == 7);
        CHECK(clade_ranges(parent, 7, inner, 4, false, o, n, l, h, &bad, err) == ST_ERR_ARG && bad == 4);
        CHECK(clade_ranges(parent, 7, rep, 4, false, o, n, l, h, &bad, err) == ST_ERR_ARG && bad == 2);
        CHECK(clade_ranges(parent, 7, ids, 3, false, o, n, l, h, &bad, err) == ST_ERR_ARG);
        CHECK(clade_ranges(nullptr, 7, ids, 4, false, o, n, l, h, &bad, err) == ST_ERR_ARG);
        const int32_t two_roots[7] = {4, 4, 5, 5, -1, 6, -1}, cycle[7] = {4, 4, 5, 5, 5, 4, -1};
        CHECK(clade_ranges(two_roots, 7, ids, 4, false, o, n, l, h, &bad, err) == ST_ERR_TREE);
        CHECK(clade_ranges(cycle, 7, ids, 4, false, o, n, l, h, &bad, err) == ST_ERR_TREE);
    }
    std::printf("sanitize clade match ok\n");
    return 0;
}
