// rank_plan.cpp -- see rank_plan.h.  Integer arithmetic over caller-supplied arrays: no GPU calls.
#include "rank_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace st {

void rank_slots(const uint32_t *occupancy, RankSlots &S)
{
    S.n_slots = 0;
    for (int b = 0; b < kRankBuckets; b++) S.slot[b] = occupancy[b] ? S.n_slots++ : -1;
}

void rank_finish(int64_t n, int64_t n_nan, int64_t distinct_x, int64_t distinct_y, i128 sxy, u128 tie_x, u128 tie_y,
                 st_rank_sums *out)
{
    *out = st_rank_sums{n, n_nan, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n_nan > 0 || n == 0) return;
    const u128 cube = (u128)(uint64_t)n * (uint64_t)n * (uint64_t)n - (uint64_t)n;      // n^3 - n < 2^93
    const u128 sxx = (cube - tie_x) / 3, syy = (cube - tie_y) / 3, uxy = (u128)sxy;
    out->distinct_x = distinct_x;
    out->distinct_y = distinct_y;
    out->sxy_lo = (uint64_t)uxy;
    out->sxy_hi = (int64_t)(uint64_t)(uxy >> 64);
    out->sxx_lo = (uint64_t)sxx;
    out->sxx_hi = (uint64_t)(sxx >> 64);
    out->syy_lo = (uint64_t)syy;
    out->syy_hi = (uint64_t)(syy >> 64);
}

namespace {

// one column: its distinct keys in order, a of each, the tie sum
struct RankColumn {
    std::vector<uint32_t> keys;
    std::vector<int32_t> a;
    u128 tie = 0;

    void build(const std::vector<uint32_t> &k)
    {
        std::vector<uint32_t> sorted(k);
        std::sort(sorted.begin(), sorted.end());
        const int64_t n = (int64_t)sorted.size();
        for (int64_t i = 0; i < n;) {
            int64_t j = i;
            while (j < n && sorted[j] == sorted[i]) j++;
            keys.push_back(sorted[i]);
            a.push_back(rank_centered(i, j - i, n));
            tie += rank_tie_term((uint64_t)(j - i));
            i = j;
        }
    }
    int32_t of(uint32_t key) const { return a[std::lower_bound(keys.begin(), keys.end(), key) - keys.begin()]; }
};

}  // namespace

int spearman_host(const float *x, const float *y, int64_t n, st_rank_sums *out, std::string &err)
{
    if (!out) { err = "out is NULL"; return ST_ERR_ARG; }
    if (n < 0) { err = "n < 0"; return ST_ERR_ARG; }
    if (n > kRankMaxPairs) { err = "ranks of " + std::to_string(n) + " pairs: at most " + std::to_string(kRankMaxPairs); return ST_ERR_ARG; }
    if (n > 0 && (!x || !y)) { err = "x or y is NULL"; return ST_ERR_ARG; }
    std::vector<uint32_t> kx((size_t)n), ky((size_t)n);
    int64_t n_nan = 0;
    for (int64_t i = 0; i < n; i++) {
        uint32_t bx, by;
        std::memcpy(&bx, x + i, 4);
        std::memcpy(&by, y + i, 4);
        if (rank_is_nan(bx) || rank_is_nan(by)) {
            n_nan++;
            continue;
        }
        kx[i] = rank_key(bx);
        ky[i] = rank_key(by);
    }
    if (n_nan > 0 || n == 0) {
        rank_finish(n, n_nan, 0, 0, 0, 0, 0, out);
        return ST_OK;
    }
    RankColumn cx, cy;
    cx.build(kx);
    cy.build(ky);
    i128 sxy = 0;
    for (int64_t i = 0; i < n; i++) sxy += (i128)((int64_t)cx.of(kx[i]) * (int64_t)cy.of(ky[i]));
    rank_finish(n, 0, (int64_t)cx.keys.size(), (int64_t)cy.keys.size(), sxy, cx.tie, cy.tie, out);
    return ST_OK;
}

}  // namespace st
