// The host side of the per-clade Hommola test (suchtree_amd/csrc/hommola_plan.cpp, keyed_perm.h) under AddressSanitizer + UBSan
// (tests/test_hommola_clades_host.py builds this with -fsanitize=address,undefined): the plan on caterpillar and random
// trees -- laminar check, maximal ranges under several caps, blocks that tile every row once, chunk cuts -- the fold
// against clade_merge in block order, every argument error, and the host form of the permutation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/hommola_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 12345;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Tree {
    std::vector<int> parent;
    std::vector<std::vector<int>> kids;
    std::vector<int> leaf_begin, leaf_count;      // per node, over the depth-first leaf order
    int n_leaves = 0;
};

static void number_leaves(Tree &T)
{
    const int n = (int)T.parent.size();
    T.kids.assign(n, {});
    int root = -1;
    for (int v = 0; v < n; v++) {
        if (T.parent[v] < 0) root = v;
        else T.kids[T.parent[v]].push_back(v);      // (increasing id order)
    }
    T.leaf_begin.assign(n, 0);
    T.leaf_count.assign(n, 0);
    std::vector<std::pair<int, int>> stack{{root, 0}};
    int pos = 0;
    while (!stack.empty()) {
        auto &[v, k] = stack.back();
        if (k == 0) T.leaf_begin[v] = pos;
        if (T.kids[v].empty()) pos++;
        if (k < (int)T.kids[v].size()) {
            const int c = T.kids[v][k++];
            stack.push_back({c, 0});
        } else {
            T.leaf_count[v] = pos - T.leaf_begin[v];
            stack.pop_back();
        }
    }
    T.n_leaves = pos;
}

static Tree caterpillar(int leaves)
{
    Tree T;      // inner nodes 0 .. leaves-2 in a chain, each with one leaf; the last with two
    T.parent.assign(2 * leaves - 1, -1);
    for (int i = 1; i < leaves - 1; i++) T.parent[i] = i - 1;
    for (int i = 0; i < leaves - 1; i++) T.parent[leaves - 1 + i] = i;
    T.parent[2 * leaves - 2] = leaves - 2;
    number_leaves(T);
    return T;
}

static Tree random_tree(int leaves)
{
    Tree T;      // grown by splitting a random leaf
    T.parent = {-1};
    std::vector<int> tips{0};
    while ((int)tips.size() < leaves) {
        const size_t k = rnd() % tips.size();
        const int v = tips[k], a = (int)T.parent.size(), b = a + 1;
        T.parent.push_back(v);
        T.parent.push_back(v);
        tips[k] = a;
        tips.push_back(b);
    }
    number_leaves(T);
    return T;
}

struct Case {
    std::vector<int32_t> pos_o, pos_c;
    std::vector<st_hommola_clade> clades;
    int n_o = 0, n_c = 0;
};

// links at random clade-tree leaves (sorted) and random other positions; the clades: inner nodes of at most max_leaves
static Case make_case(const Tree &T, int n_links, int n_o, int max_leaves)
{
    Case C;
    C.n_o = n_o;
    C.n_c = T.n_leaves;
    for (int l = 0; l < n_links; l++) C.pos_c.push_back((int32_t)(rnd() % (uint64_t)T.n_leaves));
    std::sort(C.pos_c.begin(), C.pos_c.end());
    for (int l = 0; l < n_links; l++) C.pos_o.push_back((int32_t)(rnd() % (uint64_t)n_o));
    for (int v = 0; v < (int)T.parent.size(); v++) {
        if (T.kids[v].empty() || T.leaf_count[v] > max_leaves) continue;
        const int lo = (int)(std::lower_bound(C.pos_c.begin(), C.pos_c.end(), T.leaf_begin[v]) - C.pos_c.begin());
        const int hi = (int)(std::lower_bound(C.pos_c.begin(), C.pos_c.end(), T.leaf_begin[v] + T.leaf_count[v]) - C.pos_c.begin());
        C.clades.push_back(st_hommola_clade{v, T.leaf_begin[v], T.leaf_count[v], lo, hi - lo, 0});
    }
    return C;
}

static int plan_of(const Case &C, int64_t perms, int64_t chunk_blocks, HommolaPlan &P, std::string &err)
{
    return hommola_plan(C.n_o, C.n_c, C.pos_o.data(), C.pos_c.data(), (int64_t)C.pos_o.size(), C.clades.data(), (int64_t)C.clades.size(), perms,
                        chunk_blocks, P, err);
}

static bool same(const st_pair_moments &a, const st_pair_moments &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int check_case(const Tree &T, const Case &C, int max_leaves, int64_t perms)
{
    std::string err;
    HommolaPlan P;
    CHECK(plan_of(C, perms, 0, P, err) == ST_OK);
    const int64_t R = perms + 1;
    CHECK(P.n_rows == (int64_t)C.clades.size() * R && P.rows_per_clade == R);
    // maximal ranges: the clades whose parent is not within the cap (or is no clade), disjoint and in order
    std::map<int, int> want;      // leaf_begin -> leaf_count
    for (const auto &k : C.clades) {
        const int up = T.parent[k.node];
        if (up < 0 || T.leaf_count[up] > max_leaves) want[k.leaf_begin] = k.leaf_count;
    }
    CHECK(P.ranges.size() == want.size());
    int64_t floats = (int64_t)C.n_o * C.n_o;
    size_t ri = 0;
    for (const auto &[b, n] : want) {
        CHECK(P.ranges[ri].leaf_begin == b && P.ranges[ri].leaf_count == n && P.ranges[ri].mat_off == floats);
        floats += (int64_t)n * n;
        ri++;
    }
    CHECK(P.mat_floats == floats);
    for (size_t c = 0; c < C.clades.size(); c++) {      // every clade's corner lies on its maximal matrix's diagonal
        const HommolaCladeDev &d = P.clades[c];
        bool found = false;
        for (const auto &g : P.ranges)
            if (g.leaf_begin <= d.leaf_begin && d.leaf_begin + d.leaf_count <= g.leaf_begin + g.leaf_count && g.leaf_count == d.mat_n) {
                found = d.mat_off == g.mat_off + (int64_t)(d.leaf_begin - g.leaf_begin) * (g.leaf_count + 1);
                if (found) break;
            }
        CHECK(found);
    }
    // blocks tile every row exactly once, in row order
    std::vector<int64_t> covered((size_t)P.n_rows, 0);
    int64_t prev_row = -1;
    for (int64_t t = 0; t < P.n_blocks; t++) {
        const HommolaBlock b = P.block(t);
        CHECK(b.row >= prev_row && b.row == b.clade * R + b.p && b.len >= 1 && b.len <= ST_CLADE_TILE && b.first % ST_CLADE_TILE == 0);
        CHECK(b.first == covered[(size_t)b.row]);
        covered[(size_t)b.row] += b.len;
        prev_row = b.row;
    }
    for (int64_t r = 0; r < P.n_rows; r++) {
        const int64_t L = C.clades[(size_t)(r / R)].link_count;
        CHECK(covered[(size_t)r] == L * (L - 1) / 2);
        CHECK(P.row_rel(r) == P.clades[(size_t)(r / R)].rel_begin + (r % R) * (L >= 2 ? L : 0));
    }
    // chunk cuts: whole blocks, in order, nothing left out; the rows and positions they name
    for (int64_t cb : {1, 2, 7, 0}) {
        HommolaPlan Q;
        CHECK(plan_of(C, perms, cb, Q, err) == ST_OK);
        int64_t t = 0;
        for (const HommolaChunk &k : Q.chunks) {
            CHECK(k.block_begin == t && k.n_blocks >= 1 && (cb == 0 || k.n_blocks <= cb) && k.n_blocks <= Q.max_chunk_blocks);
            CHECK(cb == 0 || k.n_blocks == cb || k.block_begin + k.n_blocks == Q.n_blocks);
            const HommolaBlock first = Q.block(t), last = Q.block(t + k.n_blocks - 1);
            CHECK(k.row_begin == first.row && k.row_begin + k.n_rows - 1 == last.row);
            CHECK(k.rel_begin == Q.row_rel(first.row) && k.rel_begin + k.n_rel == Q.row_rel(last.row) + C.clades[(size_t)last.clade].link_count);
            CHECK(k.n_rel <= Q.max_chunk_rel && k.side0_classes != 0);
            t += k.n_blocks;
        }
        CHECK(t == Q.n_blocks && Q.n_blocks == P.n_blocks);
    }
    // the fold of synthetic pieces, taken chunk by chunk, equals clade_merge in block order
    std::vector<CladePiece> pieces((size_t)P.n_blocks);
    for (auto &q : pieces) {
        const float cx = (float)(rnd() % 1000) / 7.0f, cy = (float)(rnd() % 1000) / 3.0f;
        q = CladePiece{(double)(rnd() % 100) / 9.0, (double)(rnd() % 100) / 11.0, (double)(rnd() % 1000), (double)(rnd() % 1000),
                       (double)(rnd() % 1000) - 500.0, cx, cy, cx - 1.0f, cx + 2.0f, cy - 3.0f, cy + 4.0f};
    }
    std::vector<st_pair_moments> want_rows((size_t)P.n_rows, moments_empty()), got((size_t)P.n_rows, moments_empty());
    for (int64_t t = 0; t < P.n_blocks; t++) {
        const HommolaBlock b = P.block(t);
        clade_merge(want_rows[(size_t)b.row], piece_moments(pieces[(size_t)t], b.len));
    }
    HommolaPlan Q;
    CHECK(plan_of(C, perms, 3, Q, err) == ST_OK);
    for (const HommolaChunk &k : Q.chunks) hommola_fold(Q, k.block_begin, k.n_blocks, pieces.data() + k.block_begin, got.data());
    for (int64_t r = 0; r < P.n_rows; r++) CHECK(same(want_rows[(size_t)r], got[(size_t)r]));
    return 0;
}

int main()
{
    for (int max_leaves : {184, 64, 8, 3}) {
        const Tree cat = caterpillar(184);
        if (check_case(cat, make_case(cat, 184, 35, max_leaves), max_leaves, 3)) return 1;
        const Tree rt = random_tree(300);
        if (check_case(rt, make_case(rt, 400, 40, max_leaves), max_leaves, 2)) return 1;
    }
    {      // a clade of many links: several blocks per row, the default chunk
        const Tree rt = random_tree(40);
        if (check_case(rt, make_case(rt, 700, 10, 40), 40, 1)) return 1;
    }
    {      // the cuts that tests/test_gpu_hommola_clades.py (the drain order of the last two chunks) relies on: one clade of
           // `links` links, one per leaf -> the sizes of its chunks
        auto cuts = [](int links, int64_t perms, int64_t chunk_blocks, std::vector<int64_t> &sizes) {
            Case C;
            C.n_o = 35;
            C.n_c = links;
            for (int l = 0; l < links; l++) {
                C.pos_c.push_back(l);
                C.pos_o.push_back(l % 35);
            }
            C.clades = {st_hommola_clade{0, 0, links, 0, links, 0}};
            std::string err;
            HommolaPlan P;
            if (plan_of(C, perms, chunk_blocks, P, err) != ST_OK) return false;
            sizes.clear();
            for (const HommolaChunk &k : P.chunks) sizes.push_back(k.n_blocks);
            return P.clades[0].nb == (links == 182 ? 3 : 2);
        };
        std::vector<int64_t> n;
        CHECK(cuts(182, 0, 1, n) && n == std::vector<int64_t>({1, 1, 1}));               // 16471 pairs: three blocks, an odd count
        CHECK(cuts(182, 1, 1, n) && n == std::vector<int64_t>({1, 1, 1, 1, 1, 1}));      // an even count
        CHECK(cuts(182, 0, 2, n) && n == std::vector<int64_t>({2, 1}));                  // the last row split 2 + 1
        CHECK(cuts(130, 1, 3, n) && n == std::vector<int64_t>({3, 1}));                  // two blocks per row: row 1 crosses the cut
    }
    // arguments
    {
        const Tree rt = random_tree(50);
        const Case good = make_case(rt, 80, 12, 50);
        std::string err;
        HommolaPlan P;
        CHECK(plan_of(good, 5, 0, P, err) == ST_OK);
        CHECK(plan_of(good, -1, 0, P, err) == ST_ERR_ARG && !err.empty());
        CHECK(plan_of(good, 5, -1, P, err) == ST_ERR_ARG);
        Case c = good;
        std::swap(c.pos_c[3], c.pos_c[70]);
        CHECK(c.pos_c[3] != c.pos_c[70] && plan_of(c, 5, 0, P, err) == ST_ERR_ARG);      // pos_c not non-decreasing
        c = good;
        c.pos_o[5] = 12;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                                   // a position outside its universe
        c.pos_o[5] = -1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);
        c = good;
        c.pos_c.back() = 50;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);
        c = good;
        c.clades[2].link_count++;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                                   // a link range that is not the leaf range's
        c = good;
        c.clades[2].link_begin--;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);
        c = good;
        c.clades[0].leaf_count = 51;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                                   // a leaf range outside the universe
        {      // ranges that overlap without nesting
            Case o;
            o.n_o = 5;
            o.n_c = 10;
            o.pos_c = {1, 4, 6};
            o.pos_o = {0, 1, 2};
            o.clades = {st_hommola_clade{1, 0, 6, 0, 2, 0}, st_hommola_clade{2, 3, 6, 1, 2, 0}};
            CHECK(plan_of(o, 5, 0, P, err) == ST_ERR_ARG && err.find("nesting") != std::string::npos);
            o.clades[1] = st_hommola_clade{2, 6, 4, 2, 1, 0};      // disjoint: fine
            CHECK(plan_of(o, 5, 0, P, err) == ST_OK && P.ranges.size() == 2);
            o.clades[1] = st_hommola_clade{2, 0, 6, 0, 2, 0};      // the same range twice: nested
            CHECK(plan_of(o, 5, 0, P, err) == ST_OK && P.ranges.size() == 1);
        }
        c = good;
        c.n_o = kPermMaxUniverse + 1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);                                   // a universe above the limit
        c = good;
        c.n_c = kPermMaxUniverse + 1;
        CHECK(plan_of(c, 5, 0, P, err) == ST_ERR_ARG);
        c = good;
        c.n_o = kPermMaxUniverse;
        CHECK(plan_of(c, 5, 0, P, err) == ST_OK);
        // nothing to do: no clades, no links
        CHECK(hommola_plan(3, 3, nullptr, nullptr, 0, nullptr, 0, 5, 0, P, err) == ST_OK && P.n_blocks == 0 && P.chunks.empty() && P.n_rows == 0);
        const st_hommola_clade empty{0, 0, 3, 0, 0, 0};
        CHECK(hommola_plan(3, 3, nullptr, nullptr, 0, &empty, 1, 5, 0, P, err) == ST_OK && P.n_blocks == 0 && P.n_rows == 6);
    }
    // the host permutation: a permutation, sorted keys, the identity at p = 0, its arguments
    for (int32_t n : {1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 16383, 16384}) {
        for (uint64_t seed : {0ull, 2024ull, ~0ull}) {
            std::vector<int32_t> s((size_t)n), seen((size_t)n, 0);
            perm_host(seed, 7, 3, 1, n, s.data());
            const uint64_t h1 = perm_stream(seed, 7, 3, 1);
            for (int32_t j = 0; j < n; j++) {
                CHECK(s[(size_t)j] >= 0 && s[(size_t)j] < n && seen[(size_t)s[(size_t)j]]++ == 0);
                CHECK(j == 0 || perm_key(h1, (uint32_t)s[(size_t)j - 1]) < perm_key(h1, (uint32_t)s[(size_t)j]));
            }
            perm_host(seed, 7, 0, 1, n, s.data());
            for (int32_t j = 0; j < n; j++) CHECK(s[(size_t)j] == j);
        }
    }
    {
        std::string err;
        CHECK(perm_args(0, 1, 0, 1, err) == ST_OK && perm_args(0, 1, 1, kPermMaxUniverse, err) == ST_OK);
        CHECK(perm_args(0, 1, 0, 0, err) == ST_ERR_ARG && perm_args(0, 1, 0, kPermMaxUniverse + 1, err) == ST_ERR_ARG);
        CHECK(perm_args(0, -1, 0, 4, err) == ST_ERR_ARG && perm_args(0, 1, 2, 4, err) == ST_ERR_ARG);
        CHECK(perm_args(-1, 1, 0, 4, err) == ST_ERR_ARG);
    }
    std::printf("sanitize hommola ok\n");
    return 0;
}
