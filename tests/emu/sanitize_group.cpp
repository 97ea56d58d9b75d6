// The host side of the group sums (suchtree_amd/csrc/group_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_group_tests_host.py builds this with -fsanitize=address,undefined): the plan over small and odd shapes --
// the wave form up to 64 rows, above it row pairs, slices of every length from 1 to beyond the block, chunk cuts that
// tile every block of permutations once --
// the restatement against a plain loop over the definition with the pairs in another order, the sums at the largest
// codes, labels at the top of the byte, and every argument error in the stated order.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/group_plan.h"
#include "chunks_tile.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 2727;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Case {
    int32_t n = 0, n_groups = 0;
    std::vector<int32_t> y;
    std::vector<uint8_t> group;
};

static Case make_case(int32_t n, int32_t n_groups, int extreme)
{
    Case C;
    C.n = n;
    C.n_groups = n_groups;
    C.y.resize((size_t)n * (size_t)(n - 1) / 2);
    C.group.resize((size_t)n);
    for (auto &v : C.y) v = extreme > 0 ? INT32_MAX : extreme < 0 ? INT32_MIN : (int32_t)(rnd() >> 32);
    for (auto &g : C.group) g = (uint8_t)(n_groups - 1 - (int32_t)(rnd() % (uint64_t)std::min(n_groups, 5)));      // (the top labels)
    return C;
}

static int check_case(const Case &C, int64_t perms, int64_t chunk, int32_t slice, uint64_t seed, int32_t stream)
{
    std::string err;
    GroupPlan P;
    const int32_t n = C.n, a = C.n_groups;
    std::vector<int64_t> out((size_t)(perms + 1) * (size_t)a, -1);
    CHECK(group_plan(C.y.data(), n, C.group.data(), a, perms, stream, chunk, slice, out.data(), P, err) == ST_OK);
    CHECK(P.n == n && P.n_groups == a && P.rows == perms + 1 && P.wave == (n <= kGroupWaveMax) && P.slice == slice);
    CHECK(P.items == (P.wave ? 1 : (n + 1) / 2));
    // the chunks tile every block's (row pair, slice) tasks once, in order
    if (chunks_tile(P, chunk, [&](int64_t n_perms) { return sliced_block_tasks(P, n_perms); })) return 1;
    for (const DispersionChunk &c : P.chunks) {
        const int64_t n_slices = dispersion_slices(c.n_perms, slice);
        CHECK(n_slices >= 1 && (n_slices - 1) * slice < c.n_perms && n_slices * slice >= c.n_perms);
        CHECK(sliced_block_tasks(P, c.n_perms) == (P.wave ? c.n_perms : P.items * n_slices));
    }
    CHECK(sliced_stride(n) % 16 == 0 && sliced_stride(n) >= (size_t)n && sliced_stride(n) < (size_t)n + 16);
    // the restatement against the definition, the pairs in another order
    group_host(C.y.data(), C.group.data(), P, seed, stream, out.data());
    std::vector<int32_t> sigma((size_t)n);
    for (int64_t p = 0; p <= perms; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        std::vector<int64_t> want((size_t)a, 0);
        for (int32_t j = 0; j < n; j++)
            for (int32_t i = n - 1; i > j; i--) {
                const uint8_t gi = C.group[(size_t)sigma[(size_t)i]], gj = C.group[(size_t)sigma[(size_t)j]];
                if (gi == gj) want[gi] += C.y[(size_t)i * (size_t)(i - 1) / 2 + (size_t)j];
            }
        for (int32_t h = 0; h < a; h++) CHECK(out[(size_t)p * (size_t)a + (size_t)h] == want[(size_t)h]);
    }
    return 0;
}

// the default block (chunk_tasks 0) where each of its two bounds binds, with more permutations than the bound
static int check_blocks()
{
    struct Want {
        int32_t n;
        int64_t perm_block;
    };
    for (const Want w : {Want{64, 524288} /* the sigma rows: 2^26 / (2 x 64) */, Want{65, 127100} /* row pairs x permutations: 2^22 / 33 */}) {
        const Case C = make_case(w.n, 3, 0);
        std::string err;
        GroupPlan P;
        int64_t out = 0;
        CHECK(group_plan(C.y.data(), w.n, C.group.data(), 3, 600000, 0, 0, kGroupSlice, &out, P, err) == ST_OK);
        CHECK(P.perm_block == w.perm_block);
        CHECK(w.perm_block == std::min(kDispersionSigmaBytes / (2 * w.n), kGroupBlockItems / P.items));
        if (chunks_tile(P, 0, [&](int64_t n_perms) { return sliced_block_tasks(P, n_perms); })) return 1;
    }
    return 0;
}

static int check_rows()
{
    // a row's record: the label of the row and the sum over the earlier objects that carry it
    const int32_t y[5] = {7, -3, 11, INT32_MAX, INT32_MIN};
    const uint8_t G[6] = {255, 0, 255, 255, 0, 255};
    GroupPart r = group_row(y, G, 5);
    CHECK(r.g == 255 && r.sum == 7 + 11 + (int64_t)INT32_MAX);
    r = group_row(y, G, 4);
    CHECK(r.g == 0 && r.sum == -3);
    r = group_row(y, G, 0);
    CHECK(r.g == 255 && r.sum == 0);
    return 0;
}

static int check_errors()
{
    const Case C = make_case(5, 3, 0);
    std::string err;
    GroupPlan P;
    int64_t out[12];
    auto plan = [&](const int32_t *y, const uint8_t *g, int32_t n, int32_t a, int64_t perms, int32_t stream, int64_t chunk, const int64_t *o, int32_t slice = 4) {
        return group_plan(y, n, g, a, perms, stream, chunk, slice, o, P, err);
    };
    const int32_t *y = C.y.data();
    const uint8_t *g = C.group.data();
    CHECK(plan(nullptr, nullptr, 2, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, kPermMaxUniverse + 1, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, 5, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err == "permutations < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, 3, -1, -1, nullptr) == ST_ERR_ARG && err == "chunk_tasks < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, 3, -1, 0, nullptr) == ST_ERR_ARG && err == "stream < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, (int64_t)1 << 31, 0, 0, nullptr) == ST_ERR_ARG && err.find("permutations") != std::string::npos);
    CHECK(plan(nullptr, nullptr, 5, 0, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "0 groups: 1 to 256");
    CHECK(plan(nullptr, nullptr, 5, 257, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "257 groups: 1 to 256");
    CHECK(plan(nullptr, g, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "y or group is NULL");
    CHECK(plan(y, nullptr, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "y or group is NULL");
    CHECK(plan(y, g, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "out is NULL");
    uint8_t bad[5] = {0, 1, 2, 2, 1};
    CHECK(plan(y, bad, 5, 2, 2, 0, 0, out) == ST_ERR_ARG && err == "group[2] = 2 of 2 groups");
    CHECK(plan(y, g, 5, 3, 2, 0, 0, out, 0) == ST_ERR_ARG && plan(y, g, 5, 3, 2, 0, 0, out, kGroupSliceMax + 1) == ST_ERR_ARG);
    CHECK(plan(y, g, 5, 3, 2, 0, 0, out) == ST_OK);
    return 0;
}

int main()
{
    for (int32_t n : {3, 4, 5, 64, 65, 257})
        for (int32_t a : {1, 2, 6, 256}) {
            const Case C = make_case(n, a, 0);
            const int64_t perms = n > 100 ? 2 : 5;
            if (check_case(C, perms, 0, kGroupSlice, rnd(), (int32_t)(rnd() % 1000))) return 1;
            for (int32_t slice : {1, 3, 64, kGroupSliceMax})
                for (int64_t chunk : {1, 2, 5, 40})
                    if (n < 100 && a == 6 && check_case(C, 7, chunk, slice, rnd(), 0)) return 1;
        }
    if (check_case(make_case(257, 1, 1), 2, 16, 3, 11, 0) || check_case(make_case(257, 2, -1), 2, 0, 16, 12, 0)) return 1;
    if (check_blocks() || check_rows() || check_errors()) return 1;
    std::printf("sanitize group ok\n");
    return 0;
}
