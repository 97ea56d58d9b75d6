// compare_plan.cpp -- see compare_plan.h.  Index arithmetic driven by caller-supplied parent arrays and link lists,
// and the float64 folding of pieces: no GPU calls.
#include "compare_plan.h"
#include "plan_checks.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace st {

st_pair_moments moments_empty()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    return st_pair_moments{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, nan, nan, nan};
}

st_pair_moments piece_moments(const CladePiece &c, int64_t n)
{
    return st_pair_moments{n, (double)c.cx, (double)c.cy, c.sx, c.sy, c.sxx, c.syy, c.sxy,
                           (double)c.min_x, (double)c.max_x, (double)c.min_y, (double)c.max_y};
}

void clade_merge(st_pair_moments &a, const st_pair_moments &b)
{
    if (b.n == 0) return;
    if (a.n == 0) {
        a = b;
        return;
    }
    const double dx = b.shift_x - a.shift_x, dy = b.shift_y - a.shift_y, nb = (double)b.n;
    a.sx = a.sx + b.sx + nb * dx;
    a.sy = a.sy + b.sy + nb * dy;
    // (an infinite value makes b's squares +inf about any shift: moved, they would be inf - inf = NaN where dx * b.sx < 0)
    a.sxx = std::isinf(b.sxx) ? a.sxx + b.sxx : a.sxx + b.sxx + 2.0 * dx * b.sx + nb * dx * dx;
    a.syy = std::isinf(b.syy) ? a.syy + b.syy : a.syy + b.syy + 2.0 * dy * b.sy + nb * dy * dy;
    a.sxy = a.sxy + b.sxy + dx * b.sy + dy * b.sx + nb * dx * dy;
    a.n += b.n;
    a.min_x = std::fmin(a.min_x, b.min_x);
    a.max_x = std::fmax(a.max_x, b.max_x);
    a.min_y = std::fmin(a.min_y, b.min_y);
    a.max_y = std::fmax(a.max_y, b.max_y);
}

int compare_hist_args(const double *edges_x, int32_t bins_x, const double *edges_y, int32_t bins_y, const int64_t *out_hist,
                      int64_t max_cells, std::string &err)
{
    if (!edges_x && !edges_y && !out_hist) return ST_OK;
    if (!edges_x || !edges_y || !out_hist) return fail(ST_ERR_ARG, err, "edges_x, edges_y and out_hist must all be given or all be NULL");
    if (bins_x < 1 || bins_y < 1) return fail(ST_ERR_ARG, err, "bins_x and bins_y must be >= 1");
    if ((int64_t)bins_x * bins_y > max_cells)
        return fail(ST_ERR_ARG, err, "histogram of " + std::to_string((int64_t)bins_x * bins_y) + " cells: at most " + std::to_string(max_cells));
    const double *edges[2] = {edges_x, edges_y};
    const int32_t bins[2] = {bins_x, bins_y};
    for (int a = 0; a < 2; a++) {
        const double *e = edges[a];
        for (int32_t i = 0; i <= bins[a]; i++) {
            if (!std::isfinite(e[i])) return fail(ST_ERR_ARG, err, "histogram edges must be finite");
            if (i > 0 && e[i] < e[i - 1]) return fail(ST_ERR_ARG, err, "histogram edges must be monotonically increasing");
        }
        if (!(e[0] < e[bins[a]])) return fail(ST_ERR_ARG, err, "the first histogram edge must be below the last");
    }
    return ST_OK;
}

bool ids_in_range(const int64_t *ids, int64_t n, int64_t n_nodes, long long &max_bad, long long &min_bad)
{
    bool ok = true;
    for (int64_t i = 0; i < n; i++) {
        const long long v = ids[i];
        if (v < 0 || v >= n_nodes) {
            max_bad = std::max(max_bad, v);
            min_bad = std::min(min_bad, v);
            ok = false;
        }
    }
    return ok;
}

int clade_plan(const int32_t *parent, int64_t n, const int64_t *link_leaf, int64_t L, int64_t cap, CladePlan &P,
               std::string &err)
{
    if (n < 1) return fail(ST_ERR_ARG, err, "n_nodes < 1");
    if (n > INT32_MAX || L > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 nodes or links");
    if (L < 0) return fail(ST_ERR_ARG, err, "n_links < 0");
    if (!parent || (L > 0 && !link_leaf)) return fail(ST_ERR_ARG, err, "parent or link_leaf is NULL");
    int64_t root = -1;
    P.child_off.assign(n + 1, 0);
    for (int64_t v = 0; v < n; v++) {
        const int64_t p = parent[v];
        if (p == -1) {
            if (root >= 0) return fail(ST_ERR_TREE, err, "parent array has more than one root");
            root = v;
        } else if (p < 0 || p >= n || p == v) {
            return fail(ST_ERR_TREE, err, "parent[" + std::to_string(v) + "] = " + std::to_string(p) + " is not a node");
        } else {
            P.child_off[p + 1]++;
        }
    }
    if (root < 0) return fail(ST_ERR_TREE, err, "parent array has no root");
    for (int64_t v = 0; v < n; v++) P.child_off[v + 1] += P.child_off[v];
    P.child.assign(n > 1 ? n - 1 : 0, 0);
    {
        std::vector<int64_t> fill(P.child_off.begin(), P.child_off.end() - 1);
        for (int64_t v = 0; v < n; v++)
            if (parent[v] >= 0) P.child[fill[parent[v]]++] = v;      // (increasing id order)
    }
    P.pre.clear();
    P.pre.reserve(n);
    std::vector<int64_t> stack{root};
    while (!stack.empty()) {
        const int64_t v = stack.back();
        stack.pop_back();
        P.pre.push_back(v);
        for (int64_t i = P.child_off[v + 1] - 1; i >= P.child_off[v]; i--) stack.push_back(P.child[i]);
        if ((int64_t)P.pre.size() > n) break;
    }
    if ((int64_t)P.pre.size() != n) return fail(ST_ERR_TREE, err, "parent array is not one rooted tree (a cycle or a detached node)");
    auto is_leaf = [&](int64_t v) { return P.child_off[v + 1] == P.child_off[v]; };
    // links: ids in range (as the compare calls report them), then leaves only
    long long max_bad = 0, min_bad = 0;
    if (!ids_in_range(link_leaf, L, n, max_bad, min_bad)) return ST_ERR_BOUNDS;
    P.count.assign(n, 0);
    for (int64_t j = 0; j < L; j++) {
        if (!is_leaf(link_leaf[j])) return fail(ST_ERR_ARG, err, "link " + std::to_string(j) + ": node " + std::to_string(link_leaf[j]) + " is not a leaf of the clade tree");
        P.count[link_leaf[j]]++;
    }
    // leaves in preorder get consecutive position ranges; links keep rank order within a leaf
    P.begin.assign(n, 0);
    P.leaves.assign(n, 0);
    int64_t pos = 0;
    for (const int64_t v : P.pre)
        if (is_leaf(v)) {
            P.begin[v] = pos;
            pos += P.count[v];
            P.leaves[v] = 1;
        }
    {
        std::vector<int64_t> cur(P.begin);
        P.perm.assign(L, 0);
        for (int64_t j = 0; j < L; j++) P.perm[cur[link_leaf[j]]++] = j;
    }
    for (int64_t i = n - 1; i >= 0; i--) {
        const int64_t v = P.pre[i];
        if (is_leaf(v)) continue;
        int64_t c = 0, l = 0;
        for (int64_t e = P.child_off[v]; e < P.child_off[v + 1]; e++) {
            c += P.count[P.child[e]];
            l += P.leaves[P.child[e]];
        }
        P.count[v] = c;
        P.leaves[v] = l;
        P.begin[v] = P.begin[P.child[P.child_off[v]]];
    }
    // segments
    P.segs.clear();
    P.node_seg.assign(n, 0);
    P.node_nseg.assign(n, 0);
    P.total = 0;
    auto emit = [&](int32_t kind, int64_t v, int64_t r0, int64_t r1, int64_t c0, int64_t c1, int64_t np) {
        P.segs.push_back(st_clade_segment{P.total, np, kind, (int32_t)v, (int32_t)r0, (int32_t)r1, (int32_t)c0, (int32_t)c1});
        P.total += np;
        P.node_nseg[v]++;
    };
    // nodes by link count (ties: reverse preorder), so that the segments of the nodes within any cap are a prefix of the
    // pair range and keep their pair indices -- hence their pieces and their bits -- whatever the cap
    std::vector<int64_t> order(P.pre.rbegin(), P.pre.rend());
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return P.count[a] < P.count[b]; });
    for (const int64_t v : order) {
        P.node_seg[v] = (int64_t)P.segs.size();
        if (cap >= 0 && P.count[v] > cap) continue;
        const int64_t end = P.begin[v] + P.count[v];
        if (is_leaf(v)) {
            if (P.count[v] >= 2) emit(ST_CLADE_TRI, v, P.begin[v], end, 0, 0, P.count[v] * (P.count[v] - 1) / 2);
            continue;
        }
        for (int64_t e = P.child_off[v]; e + 1 < P.child_off[v + 1]; e++) {
            const int64_t c = P.child[e], rows = P.count[c], c0 = P.begin[c] + rows;
            if (rows > 0 && end > c0) emit(ST_CLADE_RECT, v, P.begin[c], c0, c0, end, rows * (end - c0));
        }
    }
    return ST_OK;
}

bool clade_tables(const CladePlan &P, CladeTables &T)
{
    const int64_t total = P.total, n_segs = (int64_t)P.segs.size();
    const int64_t n_tiles = (total + ST_CLADE_TILE - 1) / ST_CLADE_TILE;
    T.segs.assign(n_segs + 1, CladeSeg{});
    T.tiles.assign(n_tiles + 1, CladeTile{});
    T.seg_piece.assign(n_segs + 1, 0);
    T.n_pieces = 0;
    for (int64_t s = 0; s < n_segs; s++) {
        const st_clade_segment &g = P.segs[s];
        T.segs[s] = CladeSeg{(long long)g.first_pair, g.row_begin, g.row_end, g.kind == ST_CLADE_TRI ? -1 : g.col_begin, g.col_end};
        const int64_t tf = g.first_pair >> kCladeTileShift, tl = (g.first_pair + g.n_pairs - 1) >> kCladeTileShift;
        T.seg_piece[s] = T.n_pieces;
        for (int64_t t = (g.first_pair + ST_CLADE_TILE - 1) >> kCladeTileShift; t <= tl; t++)      // tiles that start in s
            T.tiles[t] = CladeTile{(int)s, (int)(T.n_pieces + (t - tf))};
        T.n_pieces += tl - tf + 1;
    }
    T.seg_piece[n_segs] = T.n_pieces;
    T.segs[n_segs] = CladeSeg{(long long)total, 0, 0, 0, 0};
    if (T.n_pieces > INT32_MAX) return false;
    T.tiles[n_tiles] = CladeTile{(int)n_segs, (int)T.n_pieces};
    return true;
}

void clade_fold(const CladePlan &P, const CladeTables &T, const CladePiece *pieces, int64_t cap, st_pair_moments *out)
{
    const int64_t n = (int64_t)P.pre.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const st_pair_moments empty = moments_empty(), skipped{-1, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
    std::vector<st_pair_moments> seg_m(P.segs.size(), empty);
    for (size_t si = 0; si < P.segs.size(); si++) {
        const st_clade_segment &g = P.segs[si];
        const int64_t seg_end = g.first_pair + g.n_pairs;
        for (int64_t q = T.seg_piece[si]; q < T.seg_piece[si + 1]; q++) {
            // piece q of segment si: its part of tile t
            const int64_t t = (g.first_pair >> kCladeTileShift) + (q - T.seg_piece[si]);
            const int64_t lo = std::max<int64_t>(g.first_pair, t << kCladeTileShift);
            const int64_t hi = std::min<int64_t>(seg_end, (t + 1) << kCladeTileShift);
            clade_merge(seg_m[si], piece_moments(pieces[q], hi - lo));
        }
    }
    for (int64_t i = n - 1; i >= 0; i--) {      // (a node within the cap has every child within it)
        const int64_t v = P.pre[i];
        if (cap >= 0 && P.count[v] > cap) {
            out[v] = skipped;
            continue;
        }
        st_pair_moments acc = empty;
        for (int64_t e = P.child_off[v]; e < P.child_off[v + 1]; e++) clade_merge(acc, out[P.child[e]]);
        for (int64_t si = P.node_seg[v]; si < P.node_seg[v] + P.node_nseg[v]; si++) clade_merge(acc, seg_m[si]);
        out[v] = acc;
    }
}

RowsLayout rows_layout(int64_t n_rows, int64_t m, int64_t chunk_pairs)
{
    RowsLayout L;
    const int64_t C = chunk_pairs > 0 ? chunk_pairs : kCladeChunkPairs;
    L.P = m * (m - 1) / 2;
    L.nb = (L.P + ST_CLADE_TILE - 1) / ST_CLADE_TILE;
    if (L.P == 0) return L;
    if (L.P <= C / 2) {
        L.S = L.P;
        L.max_rows = std::max<int64_t>(1, std::min({n_rows, C / L.P, kRowsChunkBlocks / L.nb}));
        L.chunk = L.max_rows * L.P;
        L.max_blocks = L.max_rows * L.nb;
    } else {
        L.S = L.nb * ST_CLADE_TILE;
        L.chunk = C;
        L.max_rows = std::min(n_rows, (C - 1) / L.S + 2);
        L.max_blocks = std::min(C / ST_CLADE_TILE, n_rows * L.nb);
    }
    return L;
}

int64_t RowsLayout::block_of(int64_t g) const
{
    const int64_t r = g / S;
    return r * nb + ((g - r * S) >> kCladeTileShift);
}

int64_t RowsLayout::block_lo(int64_t t) const { return t / nb * S + t % nb * ST_CLADE_TILE; }

int64_t RowsLayout::block_len(int64_t t) const { return std::min<int64_t>((t % nb + 1) * ST_CLADE_TILE, P) - t % nb * ST_CLADE_TILE; }

}  // namespace st
