// clade_match_plan.cpp -- see clade_match_plan.h.  The range builder, the argument checks, the size windows and the
// restatement of the device reduction: no GPU calls.
#include "clade_match_plan.h"
#include "plan_checks.h"

#include <algorithm>

namespace st {

static int leaves_arg(int32_t m, std::string &err)
{
    if (m < kCladeMatchMinLeaves || m > kCladeMatchMaxLeaves)
        return fail(ST_ERR_ARG, err, "a list of " + std::to_string(m) + " leaves: " + std::to_string(kCladeMatchMinLeaves) + " to " +
                                         std::to_string(kCladeMatchMaxLeaves));
    return ST_OK;
}

int clade_ranges(const int32_t *parent, int64_t n, const int64_t *leaf_ids, int32_t m, bool rooted, std::vector<int32_t> &order,
                 std::vector<int32_t> &node, std::vector<int32_t> &lo, std::vector<int32_t> &hi, int64_t *bad_id, std::string &err)
{
    if (const int rc = leaves_arg(m, err); rc != ST_OK) return rc;
    if (n < 1) return fail(ST_ERR_ARG, err, "n_nodes < 1");
    if (n > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 nodes");
    if (!parent || !leaf_ids) return fail(ST_ERR_ARG, err, "parent or leaf_ids is NULL");
    // children in increasing id order, then the preorder: as clade_plan (compare_plan.cpp) reads a parent array
    int64_t root = -1;
    std::vector<int64_t> child_off((size_t)n + 1, 0);
    for (int64_t v = 0; v < n; v++) {
        const int64_t p = parent[v];
        if (p == -1) {
            if (root >= 0) return fail(ST_ERR_TREE, err, "parent array has more than one root");
            root = v;
        } else if (p < 0 || p >= n || p == v) {
            return fail(ST_ERR_TREE, err, "parent[" + std::to_string(v) + "] = " + std::to_string(p) + " is not a node");
        } else {
            child_off[p + 1]++;
        }
    }
    if (root < 0) return fail(ST_ERR_TREE, err, "parent array has no root");
    for (int64_t v = 0; v < n; v++) child_off[v + 1] += child_off[v];
    std::vector<int32_t> child((size_t)(n - 1), 0);
    {
        std::vector<int64_t> fill(child_off.begin(), child_off.end() - 1);
        for (int64_t v = 0; v < n; v++)
            if (parent[v] >= 0) child[fill[parent[v]]++] = (int32_t)v;
    }
    std::vector<int32_t> pre;
    pre.reserve((size_t)n);
    {
        std::vector<int32_t> stack{(int32_t)root};
        while (!stack.empty() && (int64_t)pre.size() <= n) {
            const int32_t v = stack.back();
            stack.pop_back();
            pre.push_back(v);
            for (int64_t e = child_off[v + 1] - 1; e >= child_off[v]; e--) stack.push_back(child[e]);
        }
    }
    if ((int64_t)pre.size() != n) return fail(ST_ERR_TREE, err, "parent array is not one rooted tree (a cycle or a detached node)");
    auto is_leaf = [&](int64_t v) { return child_off[v + 1] == child_off[v]; };
    // the listed leaves: ids of the tree, leaves, each once
    std::vector<int32_t> listed((size_t)n, -1);      // index in leaf_ids, or -1
    for (int32_t k = 0; k < m; k++) {
        const int64_t v = leaf_ids[k];
        if (v < 0 || v >= n) {
            if (bad_id) *bad_id = v;
            return ST_ERR_BOUNDS;
        }
        if (!is_leaf(v) || listed[v] >= 0) {
            if (bad_id) *bad_id = v;
            return fail(ST_ERR_ARG, err, "leaf_ids[" + std::to_string(k) + "]: node " + std::to_string(v) +
                                             (is_leaf(v) ? " is listed twice" : " is not a leaf"));
        }
        listed[v] = k;
    }
    // positions: the listed leaves in preorder; first[v] = listed leaves met before v, count[v] = those under v
    order.assign((size_t)m, 0);
    std::vector<int32_t> first((size_t)n, 0), count((size_t)n, 0);
    int32_t pos = 0;
    for (const int32_t v : pre) {
        first[v] = pos;
        if (listed[v] >= 0) {
            order[pos++] = listed[v];
            count[v] = 1;
        }
    }
    for (int64_t i = n - 1; i > 0; i--) count[parent[pre[i]]] += count[pre[i]];
    auto kept = [&](int32_t v) {
        if (count[v] < 2) return false;
        for (int64_t e = child_off[v]; e < child_off[v + 1]; e++)
            if (count[child[e]] == count[v]) return false;
        return true;
    };
    // breadth-first from the root, children in increasing id order: get_internal_nodes()
    node.clear();
    lo.clear();
    hi.clear();
    std::vector<char> prefix(rooted ? 0 : (size_t)m + 1, 0);      // prefix[k]: [0, k) is eligible
    std::vector<int32_t> level{(int32_t)root};
    for (size_t at = 0; at < level.size(); at++) {      // (the list grows as it is read)
        const int32_t v = level[at];
        for (int64_t e = child_off[v]; e < child_off[v + 1]; e++)
            if (count[child[e]] >= 2) level.push_back(child[e]);      // (nothing eligible below fewer than two listed leaves)
        if (!kept(v)) continue;
        const int32_t s = count[v];
        if (s > (rooted ? m - 1 : m - 2)) continue;
        node.push_back(v);
        lo.push_back(first[v]);
        hi.push_back(first[v] + s);
        if (!rooted && first[v] == 0) prefix[s] = 1;
    }
    if (!rooted) {      // [k, m) goes where [0, k) is eligible: the root's two children are one bipartition
        size_t w = 0;
        for (size_t r = 0; r < node.size(); r++) {
            if (hi[r] == m && prefix[lo[r]]) continue;
            node[w] = node[r];
            lo[w] = lo[r];
            hi[w++] = hi[r];
        }
        node.resize(w);
        lo.resize(w);
        hi.resize(w);
    }
    return ST_OK;
}

static int ranges_arg(const char *which, int32_t m, const int32_t *lo, const int32_t *hi, int32_t n, std::string &err)
{
    for (int32_t r = 0; r < n; r++)
        if (lo[r] < 0 || hi[r] <= lo[r] || hi[r] > m)
            return fail(ST_ERR_ARG, err, std::string(which) + " range " + std::to_string(r) + ": [" + std::to_string(lo[r]) + ", " +
                                             std::to_string(hi[r]) + ") of " + std::to_string(m) + " positions");
    return ST_OK;
}

int clade_match_args(int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo,
                     const int32_t *b_hi, int32_t n_b, int64_t chunk_rows, std::string &err)
{
    if (const int rc = leaves_arg(m, err); rc != ST_OK) return rc;
    if (n_a < 0 || n_b < 0) return fail(ST_ERR_ARG, err, "negative size");
    if (chunk_rows < 0) return fail(ST_ERR_ARG, err, "chunk_rows < 0");
    if (!pos_b || (n_a > 0 && (!a_lo || !a_hi)) || (n_b > 0 && (!b_lo || !b_hi))) return fail(ST_ERR_ARG, err, "pos_b or a range array is NULL");
    std::vector<char> seen((size_t)m, 0);
    for (int32_t k = 0; k < m; k++) {
        if (pos_b[k] < 0 || pos_b[k] >= m || seen[pos_b[k]])
            return fail(ST_ERR_ARG, err, "pos_b[" + std::to_string(k) + "] = " + std::to_string(pos_b[k]) + ": pos_b must be a permutation of 0 .. m - 1");
        seen[pos_b[k]] = 1;
    }
    if (const int rc = ranges_arg("A", m, a_lo, a_hi, n_a, err); rc != ST_OK) return rc;
    return ranges_arg("B", m, b_lo, b_hi, n_b, err);
}

// the row's prefix count: cum[x] = positions of the row below x in B's order, x = 0 .. m
static void row_prefix(int32_t m, const int32_t *pos_b, int32_t lo, int32_t hi, std::vector<int32_t> &cum)
{
    std::fill(cum.begin(), cum.end(), 0);
    for (int32_t k = lo; k < hi; k++) cum[pos_b[k] + 1] = 1;
    for (int32_t x = 0; x < m; x++) cum[x + 1] += cum[x];
}

void clade_match_host(int32_t m, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo,
                      const int32_t *b_hi, int32_t n_b, bool unrooted, int32_t *out_distance, int32_t *out_match, int32_t *out_intersection)
{
    std::vector<int32_t> cum((size_t)m + 1);
    for (int32_t r = 0; r < n_a; r++) {
        row_prefix(m, pos_b, a_lo[r], a_hi[r], cum);
        const int32_t sa = a_hi[r] - a_lo[r];
        uint64_t best = kCladeMatchNoKey;
        int32_t best_i = 0;
        for (int32_t c = 0; c < n_b; c++) {
            const int32_t i = cum[b_hi[c]] - cum[b_lo[c]];
            const uint64_t key = clade_match_key(clade_match_delta(sa, b_hi[c] - b_lo[c], i, m, unrooted), c);
            if (key < best) {
                best = key;
                best_i = i;
            }
        }
        out_distance[r] = best == kCladeMatchNoKey ? -1 : (int32_t)(best >> 32);
        out_match[r] = best == kCladeMatchNoKey ? -1 : (int32_t)(best & 0xFFFFFFFFu);
        out_intersection[r] = best_i;
    }
}

void clade_match_plan(int32_t m, const int32_t *a_lo, const int32_t *a_hi, int32_t n_a, const int32_t *b_lo, const int32_t *b_hi, int32_t n_b,
                      bool unrooted, int64_t chunk_rows, bool use_window, CladeMatchPlan &P)
{
    P = CladeMatchPlan{};
    P.m = m;
    P.n_a = n_a;
    P.n_b = n_b;
    P.unrooted = unrooted;
    P.chunk = chunk_rows > 0 ? chunk_rows : kCladeMatchChunkRows;
    // a counting sort by size (sizes are 1 .. m), stable; below[s] = candidates of a size below s, s = 0 .. m + 1
    std::vector<int32_t> below((size_t)m + 2, 0);
    for (int32_t c = 0; c < n_b; c++) below[(size_t)(b_hi[c] - b_lo[c]) + 1]++;
    for (int32_t s = 0; s <= m; s++) below[(size_t)s + 1] += below[(size_t)s];
    P.b_idx.resize((size_t)n_b);
    P.b_lo.resize((size_t)n_b);
    P.b_hi.resize((size_t)n_b);
    {
        std::vector<int32_t> at(below);
        for (int32_t c = 0; c < n_b; c++) {
            const int32_t to = at[(size_t)(b_hi[c] - b_lo[c])]++;
            P.b_idx[(size_t)to] = c;
            P.b_lo[(size_t)to] = b_lo[c];
            P.b_hi[(size_t)to] = b_hi[c];
        }
    }
    P.win.assign((size_t)n_a * 4, 0);
    if (!use_window) return;
    // sorted candidates of size in [x, y]
    auto span = [&](int64_t x, int64_t y, int32_t &w0, int32_t &w1) {
        w0 = below[(size_t)std::clamp<int64_t>(x, 0, (int64_t)m + 1)];
        w1 = below[(size_t)std::clamp<int64_t>(y + 1, 0, (int64_t)m + 1)];
        if (w1 < w0) w1 = w0;
    };
    for (int32_t r = 0; r < n_a; r++) {
        const int64_t sa = a_hi[r] - a_lo[r], bound = clade_match_bound((int32_t)sa, m, unrooted);
        int32_t *w = &P.win[(size_t)r * 4];
        if (bound < 1) continue;      // (a row of one leaf: nothing is below 0)
        // delta >= |sa - sb|: below `bound` only for sb within bound - 1 of sa; unrooted also >= |m - sa - sb|
        span(sa - bound + 1, sa + bound - 1, w[0], w[1]);
        if (!unrooted) continue;
        span(m - sa - bound + 1, m - sa + bound - 1, w[2], w[3]);
        if (w[2] < w[0]) {
            std::swap(w[0], w[2]);
            std::swap(w[1], w[3]);
        }
        if (w[2] <= w[1]) {      // (they meet: one window)
            w[1] = std::max(w[1], w[3]);
            w[2] = w[3] = 0;
        }
    }
}

void clade_match_windowed_host(const CladeMatchPlan &P, const int32_t *pos_b, const int32_t *a_lo, const int32_t *a_hi, int32_t *out_distance,
                               int32_t *out_match, int32_t *out_intersection)
{
    std::vector<int32_t> cum((size_t)P.m + 1);
    for (int32_t r = 0; r < P.n_a; r++) {
        row_prefix(P.m, pos_b, a_lo[r], a_hi[r], cum);
        const int32_t sa = a_hi[r] - a_lo[r], *w = &P.win[(size_t)r * 4];
        uint64_t best = kCladeMatchNoKey;
        int32_t best_i = 0;
        auto scan = [&](int32_t c0, int32_t c1) {
            for (int32_t c = c0; c < c1; c++) {
                const int32_t i = cum[P.b_hi[c]] - cum[P.b_lo[c]];
                const uint64_t key = clade_match_key(clade_match_delta(sa, P.b_hi[c] - P.b_lo[c], i, P.m, P.unrooted), P.b_idx[c]);
                if (key < best) {
                    best = key;
                    best_i = i;
                }
            }
        };
        scan(w[0], w[1]);
        scan(w[2], w[3]);
        if (best == kCladeMatchNoKey || (int32_t)(best >> 32) >= clade_match_bound(sa, P.m, P.unrooted)) scan(0, P.n_b);
        out_distance[r] = best == kCladeMatchNoKey ? -1 : (int32_t)(best >> 32);
        out_match[r] = best == kCladeMatchNoKey ? -1 : (int32_t)(best & 0xFFFFFFFFu);
        out_intersection[r] = best_i;
    }
}

}  // namespace st
