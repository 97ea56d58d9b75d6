// The host side of the swap null (suchtree_amd/csrc/swap_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_swap_null_host.py builds this with -fsanitize=address,undefined): the plan -- row_of, the words of a bit
// matrix row at the 64-column edges, the block rule, the blocks and chunks of the record call -- the serial chain's
// invariants, the wave's batched schedule against it on matrices where the prefixes are short and long, the prefix rule
// on hand-made batches, the records against dispersion_record on the table rows, and every argument error.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/swap_plan.h"

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
    std::vector<int32_t> pos;
    std::vector<int64_t> off{0};
};

static void add_set(Case &C, int k)      // k distinct positions of the universe, increasing
{
    std::vector<int32_t> all((size_t)C.n);
    for (int32_t i = 0; i < C.n; i++) all[(size_t)i] = i;
    for (int i = 0; i < k; i++) std::swap(all[(size_t)i], all[(size_t)i + rnd() % (uint64_t)(C.n - i)]);
    std::sort(all.begin(), all.begin() + k);
    C.pos.insert(C.pos.end(), all.begin(), all.begin() + k);
    C.off.push_back((int64_t)C.pos.size());
}

static int tables_args(const Case &C, int64_t p_begin, int64_t n_perms, int64_t iterations, int32_t stream, SwapPlan &S, std::string &err)
{
    return swap_tables_args(C.n, C.pos.data(), (int64_t)C.pos.size(), C.off.data(), (int64_t)C.off.size() - 1, p_begin, n_perms, iterations, stream, S, err);
}

static int check_case(const Case &C, int64_t iterations)
{
    std::string err;
    SwapPlan S;
    CHECK(tables_args(C, 0, 4, iterations, 3, S, err) == ST_OK);
    const int64_t n_sets = (int64_t)C.off.size() - 1, n_pos = (int64_t)C.pos.size();
    CHECK(S.L == C.off.back() - C.off[0] && S.e0 == C.off[0] && S.words == (C.n + 63) / 64 && (int64_t)S.row_of.size() == S.L);
    CHECK(S.chain_bytes == 2 * n_pos + 8 * n_sets * S.words);
    for (int64_t e = 0; e < S.L; e++) {
        const int32_t r = S.row_of[(size_t)e];
        CHECK(r >= 0 && r < n_sets && C.off[(size_t)r] <= S.e0 + e && S.e0 + e < C.off[(size_t)r + 1]);
    }
    CHECK(swap_block(S, 1000, 0) >= 1 && swap_block(S, 1000, 0) <= 1000 && swap_block(S, 1000, 3) == 3 && swap_block(S, 2, 3) == 2 && swap_block(S, 0, 0) == 1);
    std::vector<int> degree((size_t)C.n, 0);
    for (int64_t e = C.off[0]; e < C.off.back(); e++) degree[(size_t)C.pos[(size_t)e]]++;      // (the links)
    std::vector<uint16_t> row((size_t)std::max<int64_t>(n_pos, 1)), again(row.size());
    for (int64_t p = 0; p < 5; p++) {
        int64_t accepted = -1, accepted_b = -1, steps = 0;
        swap_chain_host(S, C.pos.data(), C.off.data(), 77, 3, p, row.data(), &accepted);
        swap_chain_host(S, C.pos.data(), C.off.data(), 77, 3, p, again.data(), &accepted_b, true, &steps);      // the wave's schedule
        CHECK(accepted == accepted_b && accepted >= 0 && accepted <= iterations && std::equal(row.begin(), row.begin() + n_pos, again.begin()));
        CHECK(p == 0 || S.L < 2 ? steps == 0 : (steps >= (iterations + kSwapBatch - 1) / kSwapBatch && steps <= iterations));
        if (p == 0) CHECK(accepted == 0);
        std::vector<int> seen((size_t)C.n, 0);
        for (int64_t e = 0; e < n_pos; e++) CHECK((e >= C.off[0] && e < C.off.back()) || row[(size_t)e] == C.pos[(size_t)e]);      // outside the links: copied
        for (int64_t r = 0; r < n_sets; r++)
            for (int64_t e = C.off[(size_t)r]; e < C.off[(size_t)r + 1]; e++) {
                CHECK(row[(size_t)e] < C.n && (e == C.off[(size_t)r] || row[(size_t)e] > row[(size_t)e - 1]));
                if (p == 0) CHECK(row[(size_t)e] == C.pos[(size_t)e]);
                seen[row[(size_t)e]]++;
            }
        CHECK(seen == degree);
    }
    // the records: dispersion_record over the table row's sets, and the plan's blocks of chains
    std::vector<float> D((size_t)C.n * (size_t)C.n);
    for (auto &v : D) v = (float)(rnd() % 4096) / 64.0f;
    for (int64_t chunk : {0, 1, 3}) {
        DispersionPlan P;
        SwapPlan T;
        CHECK(swap_dispersion_plan(C.n, C.pos.data(), n_pos, C.off.data(), n_sets, 4, iterations, 3, chunk, P, T, err) == ST_OK);
        CHECK(P.rows == 5 && P.perm_block == swap_block(T, 5, chunk) && (chunk == 0 || P.perm_block <= chunk));
        int64_t tasks = 0;
        for (const DispersionChunk &c : P.chunks) {
            CHECK(c.n_perms <= P.perm_block && c.p_begin % P.perm_block == 0 && c.n_tasks <= P.max_chunk_tasks);
            tasks += c.n_tasks;
        }
        CHECK(tasks == (int64_t)P.order.size() * 5);
        std::vector<st_dispersion_record> out((size_t)(n_sets * 5));
        std::vector<int64_t> accepted(5, -1);
        swap_dispersion_host(D.data(), P, T, C.pos.data(), C.off.data(), 77, 3, out.data(), accepted.data());
        std::vector<int32_t> q((size_t)C.n);
        for (int64_t p = 0; p < 5; p++) {
            int64_t a = -1;
            swap_chain_host(S, C.pos.data(), C.off.data(), 77, 3, p, row.data(), &a);
            CHECK(a == accepted[(size_t)p]);
            for (int64_t r = 0; r < n_sets; r++) {
                const int64_t b = C.off[(size_t)r], k = C.off[(size_t)r + 1] - b;
                for (int64_t i = 0; i < k; i++) q[(size_t)i] = row[(size_t)(b + i)];
                const st_dispersion_record want = dispersion_record(D.data(), C.n, q.data(), (int32_t)k);
                CHECK(std::memcmp(&want, &out[(size_t)(r * 5 + p)], sizeof want) == 0);
            }
        }
    }
    return 0;
}

int main()
{
    {      // the prefix rule on hand-made batches
        const int32_t a1[5] = {0, 2, 4, 6, 8}, a2[5] = {1, 3, 5, 7, 9};
        CHECK(swap_prefix(a1, a2, 5) == 5 && swap_prefix(a1, a2, 1) == 1 && swap_prefix(a1, a2, 0) == 0);
        const int32_t b1[5] = {0, 2, 4, 1, 8}, b2[5] = {1, 3, 5, 7, 2};
        CHECK(swap_prefix(b1, b2, 5) == 3 && swap_prefix(b1, b2, 3) == 3);      // lane 3 meets lane 0 in its first row
        const int32_t c1[3] = {4, 4, 0}, c2[3] = {4, 9, 4};
        CHECK(swap_prefix(c1, c2, 3) == 1);                                    // a lane whose two rows are one row still holds it
        const int32_t d1[3] = {0, 2, 9}, d2[3] = {1, 3, 3};
        CHECK(swap_prefix(d1, d2, 3) == 2);                                    // ... in its second row
        CHECK(swap_rows_meet(1, 2, 3, 1) && swap_rows_meet(1, 2, 2, 3) && !swap_rows_meet(1, 2, 3, 4));
    }
    for (int32_t n : {3, 63, 64, 65, 128, 129, 300}) {
        Case C;
        C.n = n;
        for (int k : {0, 1, 2, 3, 5, 1, 17, 0, 64, 65, 1, 130})
            if (k <= n) add_set(C, k);
        add_set(C, n);      // the whole universe: never swaps
        add_set(C, 2);
        for (int64_t iterations : {0, 1, 63, 64, 65, 3000})
            if (check_case(C, iterations)) return 1;
    }
    {      // two rows: short prefixes; a hub row that holds half the links; many short rows
        Case two, hub, many;
        two.n = hub.n = many.n = 100;
        add_set(two, 30);
        add_set(two, 45);
        add_set(hub, 50);
        for (int i = 0; i < 50; i++) add_set(hub, 1);
        for (int i = 0; i < 300; i++) add_set(many, 1 + (int)(rnd() % 5));
        for (const Case *C : {&two, &hub, &many})
            if (check_case(*C, 2000)) return 1;
        SwapPlan S;
        std::string err;
        CHECK(tables_args(two, 0, 1, 2000, 0, S, err) == ST_OK);
        std::vector<uint16_t> row(two.pos.size());
        int64_t steps = 0, accepted = 0;
        swap_chain_host(S, two.pos.data(), two.off.data(), 1, 0, 1, row.data(), &accepted, true, &steps);
        // a second lane escapes the first only if each draws one row twice, the two rows differing: at most 2 * (1/4) * (1/4) of the
        // batches, and no third lane can follow.  So a prefix is 1 or 2 trials, and 2 in at most an eighth of the steps.
        CHECK(steps * 2 >= 2000 && steps <= 2000 && steps * 4 > 3 * 2000 && accepted > 0);
    }
    {      // nothing to swap: no sets, empty sets only, one link
        Case C;
        C.n = 5;
        if (check_case(C, 100)) return 1;
        add_set(C, 0);
        add_set(C, 0);
        if (check_case(C, 100)) return 1;
        add_set(C, 1);
        if (check_case(C, 100)) return 1;
    }
    {      // sets that begin behind the first position: the links are entries sets[0] .. sets[n_sets]
        Case C;
        C.n = 20;
        for (int k : {3, 4, 5, 2}) add_set(C, k);
        Case D = C;
        D.off.erase(D.off.begin());      // the first set's positions stay in set_pos, outside the links
        if (check_case(D, 500)) return 1;
    }
    // arguments
    {
        Case good;
        good.n = 40;
        for (int k : {3, 7, 40, 1}) add_set(good, k);
        std::string err;
        SwapPlan S;
        CHECK(tables_args(good, 0, 5, 10, 0, S, err) == ST_OK);
        CHECK(tables_args(good, -1, -1, -1, -1, S, err) == ST_ERR_ARG && err == "p_begin < 0");
        CHECK(tables_args(good, 0, -1, -1, -1, S, err) == ST_ERR_ARG && err == "n_perms < 0");
        CHECK(tables_args(good, 0, 5, -1, -1, S, err) == ST_ERR_ARG && err == "stream < 0");
        CHECK(tables_args(good, 0, 5, -1, 0, S, err) == ST_ERR_ARG && err == "iterations < 0");
        CHECK(tables_args(good, INT64_MAX, 5, 1, 0, S, err) == ST_ERR_ARG);
        Case c = good;
        c.n = 2;
        CHECK(tables_args(c, -1, 5, -1, 0, S, err) == ST_ERR_ARG && err.find("universe") != std::string::npos);
        c = good;
        std::swap(c.pos[3], c.pos[4]);
        CHECK(tables_args(c, 0, 5, -1, 0, S, err) == ST_ERR_ARG && err.find("increasing") != std::string::npos);      // the set table before iterations
        DispersionPlan P;
        CHECK(swap_dispersion_plan(40, good.pos.data(), (int64_t)good.pos.size(), good.off.data(), 4, -1, -1, 0, 0, P, S, err) == ST_ERR_ARG && err == "permutations < 0");
        CHECK(swap_dispersion_plan(40, good.pos.data(), (int64_t)good.pos.size(), good.off.data(), 4, 5, -1, 0, 0, P, S, err) == ST_ERR_ARG && err == "iterations < 0");
        // a single chain beyond the work budget: rows cost 8 words bytes each even where they are empty
        const int64_t rows = kSwapStateBytes / (8 * 256) + 1;
        std::vector<int64_t> off((size_t)rows + 1, 0);
        CHECK(swap_plan(16384, 0, off.data(), rows, 1, S, err) == ST_ERR_ARG && err.find(std::to_string(rows * 2048) + " bytes") != std::string::npos);
        CHECK(swap_plan(16384, 0, off.data(), rows - 1, 1, S, err) == ST_OK && S.chain_bytes == kSwapStateBytes && swap_block(S, 10, 0) == 1);
        CHECK(swap_plan(16384, 0, off.data(), rows, -1, S, err) == ST_ERR_ARG && err == "iterations < 0");      // iterations first
    }
    std::printf("sanitize swap ok\n");
    return 0;
}
