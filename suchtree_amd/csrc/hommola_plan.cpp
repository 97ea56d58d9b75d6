// hommola_plan.cpp -- see hommola_plan.h.  Index arithmetic driven by caller-supplied positions and clade ranges and the
// float64 folding of pieces: no GPU calls.
#include "hommola_plan.h"
#include "plan_checks.h"

#include <algorithm>
#include <numeric>

namespace st {

int hommola_plan(int32_t n_univ_o, int32_t n_univ_c, const int32_t *pos_o, const int32_t *pos_c, int64_t n_links,
                 const st_hommola_clade *clades, int64_t n_clades, int64_t permutations, int64_t chunk_blocks, HommolaPlan &P,
                 std::string &err)
{
    if (n_univ_o < 0 || n_univ_c < 0 || n_links < 0 || n_clades < 0) return fail(ST_ERR_ARG, err, "negative size");
    if (n_univ_o > kPermMaxUniverse || n_univ_c > kPermMaxUniverse)
        return fail(ST_ERR_ARG, err, "universes of " + std::to_string(n_univ_o) + " and " + std::to_string(n_univ_c) + " leaves: at most " +
                                         std::to_string(kPermMaxUniverse) + " each");
    if (permutations < 0) return fail(ST_ERR_ARG, err, "permutations < 0");
    if (chunk_blocks < 0) return fail(ST_ERR_ARG, err, "chunk_blocks < 0");
    if (n_links > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 links");
    if ((n_links > 0 && (!pos_o || !pos_c)) || (n_clades > 0 && !clades)) return fail(ST_ERR_ARG, err, "pos_o, pos_c or clades is NULL");
    for (int64_t l = 0; l < n_links; l++) {
        if (pos_o[l] < 0 || pos_o[l] >= n_univ_o || pos_c[l] < 0 || pos_c[l] >= n_univ_c)
            return fail(ST_ERR_ARG, err, "link " + std::to_string(l) + ": a position outside its universe");
        if (l > 0 && pos_c[l] < pos_c[l - 1]) return fail(ST_ERR_ARG, err, "pos_c must be non-decreasing (link " + std::to_string(l) + ")");
    }
    for (int64_t c = 0; c < n_clades; c++) {
        const st_hommola_clade &k = clades[c];
        if (k.node < 0 || k.leaf_begin < 0 || k.leaf_count < 0 || (int64_t)k.leaf_begin + k.leaf_count > n_univ_c)
            return fail(ST_ERR_ARG, err, "clade " + std::to_string(c) + ": its leaf range lies outside the universe");
        const int64_t lo = std::lower_bound(pos_c, pos_c + n_links, k.leaf_begin) - pos_c;
        const int64_t hi = std::lower_bound(pos_c, pos_c + n_links, k.leaf_begin + k.leaf_count) - pos_c;
        if (k.link_begin != lo || k.link_count != hi - lo)
            return fail(ST_ERR_ARG, err, "clade " + std::to_string(c) + ": links [" + std::to_string(k.link_begin) + ", " +
                                             std::to_string((int64_t)k.link_begin + k.link_count) + ") are not the links inside its leaf range, [" +
                                             std::to_string(lo) + ", " + std::to_string(hi) + ")");
    }
    const int64_t R = permutations + 1;
    if (n_clades > 0 && R > ((int64_t)1 << 40) / n_clades) return fail(ST_ERR_ARG, err, "more than 2^40 rows in one call");
    P = HommolaPlan{};
    P.n_clades = n_clades;
    P.rows_per_clade = R;
    P.n_rows = n_clades * R;
    P.n_univ_o = n_univ_o;
    P.n_univ_c = n_univ_c;
    P.clades.assign((size_t)n_clades + 1, HommolaCladeDev{});
    // laminar ranges: by (leaf_begin, larger first), every range must end inside the open range around it
    std::vector<int64_t> order((size_t)n_clades);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (clades[a].leaf_begin != clades[b].leaf_begin) return clades[a].leaf_begin < clades[b].leaf_begin;
        return clades[a].leaf_count > clades[b].leaf_count;
    });
    P.mat_floats = (int64_t)n_univ_o * n_univ_o;
    std::vector<int64_t> open_end;
    for (const int64_t c : order) {
        const int64_t b = clades[c].leaf_begin, e = b + clades[c].leaf_count;
        while (!open_end.empty() && open_end.back() <= b) open_end.pop_back();
        if (!open_end.empty() && e > open_end.back())
            return fail(ST_ERR_ARG, err, "clade " + std::to_string(c) + ": leaf range [" + std::to_string(b) + ", " + std::to_string(e) +
                                             ") overlaps another clade's without nesting");
        if (open_end.empty()) {
            P.ranges.push_back(HommolaRange{(int32_t)b, (int32_t)(e - b), P.mat_floats});
            P.mat_floats += (e - b) * (e - b);
        }
        open_end.push_back(e);
        const HommolaRange &r = P.ranges.back();
        HommolaCladeDev &d = P.clades[(size_t)c];
        d.mat_off = r.mat_off + (b - r.leaf_begin) * ((int64_t)r.leaf_count + 1);
        d.mat_n = r.leaf_count;
    }
    int64_t blocks = 0, rel = 0;
    for (int64_t c = 0; c < n_clades; c++) {
        const st_hommola_clade &k = clades[c];
        HommolaCladeDev &d = P.clades[(size_t)c];
        const int64_t L = k.link_count, np = L * (L - 1) / 2;
        d.block_begin = blocks;
        d.rel_begin = rel;
        d.node = k.node;
        d.leaf_begin = k.leaf_begin;
        d.leaf_count = k.leaf_count;
        d.link_begin = k.link_begin;
        d.link_count = k.link_count;
        d.nb = (int)((np + ST_CLADE_TILE - 1) / ST_CLADE_TILE);
        blocks += (int64_t)d.nb * R;
        rel += (L >= 2 ? L : 0) * R;
    }
    P.clades[(size_t)n_clades].block_begin = blocks;
    P.clades[(size_t)n_clades].rel_begin = rel;
    P.n_blocks = blocks;
    P.n_rel = rel;
    // chunks of whole blocks
    const int64_t cap_blocks = chunk_blocks > 0 ? chunk_blocks : kRowsChunkBlocks;
    const int64_t cap_pairs = chunk_blocks > 0 ? INT64_MAX : kCladeChunkPairs;
    int64_t t = 0;
    while (t < blocks) {
        int64_t n = 0, pairs = 0;
        int64_t c = P.clade_of_block(t);
        while (t + n < blocks && n < cap_blocks && pairs < cap_pairs) {
            const HommolaCladeDev &d = P.clades[(size_t)c];
            const int64_t end = P.clades[(size_t)c + 1].block_begin;
            if (t + n >= end) {
                c++;
                continue;
            }
            const int64_t L = d.link_count, np = L * (L - 1) / 2;
            const int64_t b = (t + n - d.block_begin) % d.nb;                                     // block b of its row
            int64_t take = std::min<int64_t>(d.nb - b, cap_blocks - n);                            // up to the end of the row
            if (cap_pairs != INT64_MAX) take = std::min<int64_t>(take, (cap_pairs - pairs + ST_CLADE_TILE - 1) / ST_CLADE_TILE);
            pairs += std::min<int64_t>((b + take) * ST_CLADE_TILE, np) - b * ST_CLADE_TILE;
            n += take;
        }
        const HommolaBlock first = P.block(t), last = P.block(t + n - 1);
        HommolaChunk k{};
        k.block_begin = t;
        k.n_blocks = n;
        k.row_begin = first.row;
        k.n_rows = last.row - first.row + 1;
        k.rel_begin = P.row_rel(first.row);
        k.n_rel = P.row_rel(last.row) + P.clades[(size_t)last.clade].link_count - k.rel_begin;
        for (int64_t q = first.clade; q <= last.clade; q++)
            if (P.clades[(size_t)q].link_count >= 2) k.side0_classes |= 1u << perm_sort_class(P.clades[(size_t)q].leaf_count);
        P.chunks.push_back(k);
        P.max_chunk_blocks = std::max(P.max_chunk_blocks, n);
        P.max_chunk_rel = std::max(P.max_chunk_rel, k.n_rel);
        t += n;
    }
    return ST_OK;
}

int64_t HommolaPlan::clade_of_block(int64_t t) const
{
    const auto it = std::upper_bound(clades.begin(), clades.end(), t, [](int64_t v, const HommolaCladeDev &d) { return v < d.block_begin; });
    return (int64_t)(it - clades.begin()) - 1;
}

HommolaBlock HommolaPlan::block(int64_t t) const
{
    const int64_t c = clade_of_block(t);
    const HommolaCladeDev &d = clades[(size_t)c];
    const int64_t in = t - d.block_begin, p = in / d.nb, b = in - p * d.nb;
    const int64_t L = d.link_count, np = L * (L - 1) / 2;
    return HommolaBlock{c, p, c * rows_per_clade + p, b * ST_CLADE_TILE, std::min<int64_t>((b + 1) * ST_CLADE_TILE, np) - b * ST_CLADE_TILE};
}

int64_t HommolaPlan::row_rel(int64_t row) const
{
    const int64_t c = row / rows_per_clade, p = row - c * rows_per_clade;
    const HommolaCladeDev &d = clades[(size_t)c];
    return d.rel_begin + p * (d.link_count >= 2 ? d.link_count : 0);
}

void hommola_fold(const HommolaPlan &P, int64_t block_begin, int64_t n, const CladePiece *pieces, st_pair_moments *out)
{
    if (n <= 0) return;
    int64_t c = P.clade_of_block(block_begin);
    for (int64_t j = 0; j < n; j++) {
        const int64_t t = block_begin + j;
        while (t >= P.clades[(size_t)c + 1].block_begin) c++;
        const HommolaCladeDev &d = P.clades[(size_t)c];
        const int64_t in = t - d.block_begin, p = in / d.nb, b = in - p * d.nb;
        const int64_t L = d.link_count, np = L * (L - 1) / 2;
        clade_merge(out[c * P.rows_per_clade + p], piece_moments(pieces[j], std::min<int64_t>((b + 1) * ST_CLADE_TILE, np) - b * ST_CLADE_TILE));
    }
}

}  // namespace st
