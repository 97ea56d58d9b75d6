// swap_plan.cpp -- see swap_plan.h.  Argument checks, the layout of a chain's state and the restatement of the chain
// trial for trial, in the serial order that defines it and in the wave's batched schedule: no GPU calls.
#include "swap_plan.h"
#include "plan_checks.h"

namespace st {

int swap_plan(int32_t n_univ, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t iterations, SwapPlan &P, std::string &err)
{
    if (iterations < 0) return fail(ST_ERR_ARG, err, "iterations < 0");
    P = SwapPlan{};
    P.n_univ = n_univ;
    P.n_pos = n_pos;
    P.n_sets = n_sets;
    P.iterations = iterations;
    P.e0 = n_sets > 0 ? sets[0] : 0;
    P.L = n_sets > 0 ? sets[n_sets] - sets[0] : 0;
    P.words = ((int64_t)n_univ + 63) / 64;
    P.table_bytes = n_pos * 2;
    const bool huge = n_sets > ((int64_t)1 << 40);      // (empty sets cost no positions: n_sets is not bounded by n_pos; below, no overflow)
    P.chain_bytes = huge ? INT64_MAX : P.table_bytes + n_sets * P.words * 8;
    if (P.chain_bytes > kSwapStateBytes)
        return fail(ST_ERR_ARG, err, "the state of one chain (a table row and a bit matrix of " + std::to_string(n_sets) + " x " +
                                         std::to_string(P.words * 64) + " bits) is " + (huge ? "more than " + std::to_string(kSwapStateBytes) : std::to_string(P.chain_bytes)) +
                                         " bytes: the work budget is " + std::to_string(kSwapStateBytes));
    P.row_of.resize((size_t)P.L);
    for (int64_t r = 0; r < n_sets; r++) std::fill(P.row_of.begin() + (sets[r] - P.e0), P.row_of.begin() + (sets[r + 1] - P.e0), (int32_t)r);
    return ST_OK;
}

int64_t swap_block(const SwapPlan &P, int64_t rows, int64_t chunk_tasks)
{
    int64_t block = std::max<int64_t>(1, kSwapStateBytes / std::max<int64_t>(P.chain_bytes, 1));      // (no sets: no bytes)
    if (chunk_tasks > 0) block = std::min(block, chunk_tasks);
    return std::min(block, std::max<int64_t>(rows, 1));
}

namespace {

struct Chain {
    const SwapPlan &P;
    std::vector<int32_t> col;
    std::vector<uint64_t> bits;
    int64_t accepted = 0;

    Chain(const SwapPlan &plan, const int32_t *set_pos) : P(plan), col(set_pos + plan.e0, set_pos + plan.e0 + plan.L), bits((size_t)(plan.n_sets * plan.words), 0)
    {
        for (int64_t e = 0; e < P.L; e++) flip(P.row_of[(size_t)e], col[(size_t)e]);
    }
    bool has(int32_t r, int32_t c) const { return (bits[(size_t)(r * P.words + (c >> 6))] >> (c & 63)) & 1; }
    void flip(int32_t r, int32_t c) { bits[(size_t)(r * P.words + (c >> 6))] ^= (uint64_t)1 << (c & 63); }
    void trial(int64_t e1, int64_t e2)
    {
        const int32_t r1 = P.row_of[(size_t)e1], r2 = P.row_of[(size_t)e2], b = col[(size_t)e1], d = col[(size_t)e2];
        if (r1 == r2 || b == d || has(r1, d) || has(r2, b)) return;
        flip(r1, b);
        flip(r1, d);
        flip(r2, d);
        flip(r2, b);
        col[(size_t)e1] = d;
        col[(size_t)e2] = b;
        accepted++;
    }
};

}  // namespace

void swap_chain_host(const SwapPlan &P, const int32_t *set_pos, const int64_t *sets, uint64_t seed, int32_t stream, int64_t p, uint16_t *row,
                     int64_t *accepted, bool batched, int64_t *steps)
{
    for (int64_t e = 0; e < P.n_pos; e++) row[e] = (uint16_t)set_pos[e];
    if (accepted) *accepted = 0;
    if (p == 0 || P.L < 2) return;
    Chain C(P, set_pos);
    const uint64_t h1 = perm_stream(seed, stream, p, 1);
    const int64_t T = P.iterations;
    if (!batched) {
        for (int64_t t = 0; t < T; t++) {
            int64_t e1, e2;
            swap_draw(h1, t, (uint64_t)P.L, e1, e2);
            C.trial(e1, e2);
        }
    } else {
        for (int64_t t0 = 0; t0 < T;) {
            const int n = (int)std::min<int64_t>(kSwapBatch, T - t0);
            int64_t e1[kSwapBatch], e2[kSwapBatch];
            int32_t r1[kSwapBatch], r2[kSwapBatch];
            for (int i = 0; i < n; i++) {
                swap_draw(h1, t0 + i, (uint64_t)P.L, e1[i], e2[i]);
                r1[i] = P.row_of[(size_t)e1[i]];
                r2[i] = P.row_of[(size_t)e2[i]];
            }
            const int f = swap_prefix(r1, r2, n);
            for (int i = f - 1; i >= 0; i--) C.trial(e1[i], e2[i]);      // (any order: the lanes of a prefix touch disjoint rows)
            t0 += f;
            if (steps) ++*steps;
        }
    }
    for (int64_t r = 0; r < P.n_sets; r++) {      // the rows read off in order
        int64_t e = sets[r];
        for (int64_t w = 0; w < P.words; w++)
            for (uint64_t v = C.bits[(size_t)(r * P.words + w)]; v; v &= v - 1) row[e++] = (uint16_t)(w * 64 + __builtin_ctzll(v));
    }
    if (accepted) *accepted = C.accepted;
}

int swap_tables_args(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t p_begin, int64_t n_perms,
                     int64_t iterations, int32_t stream, SwapPlan &P, std::string &err)
{
    if (n_univ < 3 || n_univ > kPermMaxUniverse)
        return fail(ST_ERR_ARG, err, "a universe of " + std::to_string(n_univ) + " positions: 3 to " + std::to_string(kPermMaxUniverse));
    if (p_begin < 0) return fail(ST_ERR_ARG, err, "p_begin < 0");
    if (n_perms < 0) return fail(ST_ERR_ARG, err, "n_perms < 0");
    if (stream < 0) return fail(ST_ERR_ARG, err, "stream < 0");
    if (p_begin > INT64_MAX - n_perms) return fail(ST_ERR_ARG, err, "p_begin + n_perms overflows");
    if (const int rc = position_sets_args(n_univ, set_pos, n_pos, sets, n_sets, err); rc != ST_OK) return rc;
    return swap_plan(n_univ, n_pos, sets, n_sets, iterations, P, err);
}

int swap_dispersion_plan(int32_t n_univ, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, int64_t permutations,
                         int64_t iterations, int32_t stream, int64_t chunk_tasks, DispersionPlan &P, SwapPlan &S, std::string &err)
{
    if (const int rc = dispersion_plan(n_univ, set_pos, n_pos, sets, n_sets, permutations, stream, chunk_tasks, P, err); rc != ST_OK) return rc;
    if (const int rc = swap_plan(n_univ, n_pos, sets, n_sets, iterations, S, err); rc != ST_OK) return rc;
    P.chunks.clear();
    P.max_chunk_tasks = 0;
    dispersion_cut_blocks(P.rows, (int64_t)P.order.size(), swap_block(S, P.rows, chunk_tasks), chunk_tasks, P.perm_block, P.chunks, P.max_chunk_tasks);
    return ST_OK;
}

void swap_dispersion_host(const float *D, const DispersionPlan &P, const SwapPlan &S, const int32_t *set_pos, const int64_t *sets, uint64_t seed,
                          int32_t stream, st_dispersion_record *out, int64_t *accepted)
{
    std::vector<uint16_t> row((size_t)std::max<int64_t>(S.n_pos, 1));
    std::vector<int32_t> q((size_t)std::max(P.max_count, 1));
    for (int64_t p = 0; p < P.rows; p++) {
        swap_chain_host(S, set_pos, sets, seed, stream, p, row.data(), accepted ? accepted + p : nullptr);      // (one randomised matrix serves every set)
        for (int64_t r = 0; r < P.n_sets; r++) {
            const int64_t b = sets[r], k = sets[r + 1] - b;
            for (int64_t i = 0; i < k && k >= 2; i++) q[(size_t)i] = row[(size_t)(b + i)];
            out[r * P.rows + p] = dispersion_record(D, P.n_univ, q.data(), (int32_t)k);
        }
    }
}

}  // namespace st
