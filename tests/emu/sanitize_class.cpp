// The host side of the class sums (suchtree_amd/csrc/class_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_correlogram_host.py builds this with -fsanitize=address,undefined): the plan over small and odd shapes --
// the wave form up to 64 rows, above it row pairs, slices of every length from 1 to beyond the block, chunk cuts that
// tile every block of permutations once, the bound of a block's partial sums --
// the restatement against a plain loop over the definition with the pairs in another order and the square written out,
// the sums at the largest codes, class 63 beside ST_CLASS_NONE, and every argument error in the stated order.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/class_plan.h"
#include "chunks_tile.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 2626;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

struct Case {
    int32_t n = 0, n_classes = 0;
    std::vector<int32_t> y;
    std::vector<uint8_t> cls;
};

static Case make_case(int32_t n, int32_t n_classes, int extreme)
{
    Case C;
    C.n = n;
    C.n_classes = n_classes;
    const size_t m = (size_t)n * (size_t)(n - 1) / 2;
    C.y.resize(m);
    C.cls.resize(m);
    for (auto &v : C.y) v = extreme > 0 ? INT32_MAX : extreme < 0 ? INT32_MIN : (int32_t)(rnd() >> 32);
    for (auto &c : C.cls) {      // (the top classes, and one pair in six in no class)
        const uint64_t r = rnd();
        c = (r % 6 == 0 && !extreme) ? (uint8_t)kClassNone : (uint8_t)(n_classes - 1 - (int32_t)((r >> 8) % (uint64_t)std::min(n_classes, 5)));
    }
    return C;
}

static int check_case(const Case &C, int64_t perms, int64_t chunk, int32_t slice, uint64_t seed, int32_t stream)
{
    std::string err;
    ClassPlan P;
    const int32_t n = C.n, K = C.n_classes;
    std::vector<int64_t> out((size_t)(perms + 1) * (size_t)K, -1);
    CHECK(class_plan(C.y.data(), C.cls.data(), n, K, perms, stream, chunk, slice, out.data(), P, err) == ST_OK);
    CHECK(P.n == n && P.n_classes == K && P.rows == perms + 1 && P.wave == (n <= kClassWaveMax) && P.slice == slice);
    CHECK(P.items == (P.wave ? 1 : (n + 1) / 2));
    CHECK(P.wave || P.perm_block * P.items * K * 8 <= kClassPartBytes);
    // the chunks tile every block's (row pair, slice) tasks once, in order
    if (chunks_tile(P, chunk, [&](int64_t n_perms) { return sliced_block_tasks(P, n_perms); })) return 1;
    for (const DispersionChunk &c : P.chunks) {
        const int64_t n_slices = dispersion_slices(c.n_perms, slice);
        CHECK(n_slices >= 1 && (n_slices - 1) * slice < c.n_perms && n_slices * slice >= c.n_perms);
        CHECK(sliced_block_tasks(P, c.n_perms) == (P.wave ? c.n_perms : P.items * n_slices));
    }
    CHECK(sliced_stride(n) % 16 == 0 && sliced_stride(n) >= (size_t)n && sliced_stride(n) < (size_t)n + 16);
    // the restatement against the definition: the square written out, the pairs in another order
    class_host(C.y.data(), C.cls.data(), P, seed, stream, out.data());
    std::vector<uint8_t> sq((size_t)n * (size_t)n, (uint8_t)kClassNone);
    for (int32_t i = 1; i < n; i++)
        for (int32_t j = 0; j < i; j++) sq[(size_t)i * n + j] = sq[(size_t)j * n + i] = C.cls[(size_t)i * (size_t)(i - 1) / 2 + (size_t)j];
    std::vector<int32_t> sigma((size_t)n);
    for (int64_t p = 0; p <= perms; p++) {
        perm_host(seed, stream, p, 0, n, sigma.data());
        std::vector<int64_t> want((size_t)K, 0);
        for (int32_t j = 0; j < n; j++)
            for (int32_t i = n - 1; i > j; i--) {
                const uint8_t c = sq[(size_t)sigma[(size_t)i] * n + (size_t)sigma[(size_t)j]];
                if (c != kClassNone) want[c] += C.y[(size_t)i * (size_t)(i - 1) / 2 + (size_t)j];
            }
        for (int32_t c = 0; c < K; c++) CHECK(out[(size_t)p * (size_t)K + (size_t)c] == want[(size_t)c]);
    }
    return 0;
}

// the default block (chunk_tasks 0) where each of its two bounds binds, with more permutations than the bound
static int check_blocks()
{
    struct Want {
        int32_t K;
        int64_t perm_block;
    };
    for (const Want w : {Want{1, 516222} /* the sigma rows: 2^26 / (2 x 65) */, Want{64, 15887} /* the partial sums: 2^28 / (8 x 64 classes x 33 row pairs) */}) {
        const Case C = make_case(65, w.K, 0);
        std::string err;
        ClassPlan P;
        int64_t out = 0;
        CHECK(class_plan(C.y.data(), C.cls.data(), 65, w.K, 600000, 0, 0, kClassSlice, &out, P, err) == ST_OK);
        CHECK(P.perm_block == w.perm_block);
        CHECK(w.perm_block == std::min(kDispersionSigmaBytes / (2 * 65), kClassPartBytes / (8 * w.K * P.items)));
        if (chunks_tile(P, 0, [&](int64_t n_perms) { return sliced_block_tasks(P, n_perms); })) return 1;
    }
    return 0;
}

static int check_rows()
{
    // a row's sums: row 3 of four objects under the relabelling (2, 0, 3, 1); pairs (1, 2), (1, 0), (1, 3) of the classes
    const int32_t y[3] = {7, INT32_MAX, INT32_MIN};
    const uint8_t cls[6] = {/* (1,0) */ 63, /* (2,0) */ 0, /* (2,1) */ 255, /* (3,0) */ 1, /* (3,1) */ 63, /* (3,2) */ 2};
    const int32_t sigma[4] = {2, 0, 3, 1};
    int64_t acc[64] = {};
    class_row(y, cls, sigma, 3, acc);
    CHECK(acc[63] == (int64_t)INT32_MAX + INT32_MIN && acc[0] == 0 && acc[1] == 0 && acc[2] == 0);      // (pair (1, 2) is in no class)
    class_row(y, cls, sigma, 0, acc);
    CHECK(acc[63] == -1);
    CHECK(class_pair(3, 1) == 4 && class_pair(1, 3) == 4 && class_pair(16383, 16382) == (size_t)16384 * 16383 / 2 - 1);
    return 0;
}

static int check_errors()
{
    const Case C = make_case(5, 3, 0);
    std::string err;
    ClassPlan P;
    int64_t out[12];
    auto plan = [&](const int32_t *y, const uint8_t *c, int32_t n, int32_t K, int64_t perms, int32_t stream, int64_t chunk, const int64_t *o, int32_t slice = 4) {
        return class_plan(y, c, n, K, perms, stream, chunk, slice, o, P, err);
    };
    const int32_t *y = C.y.data();
    const uint8_t *c = C.cls.data();
    CHECK(plan(nullptr, nullptr, 2, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, kPermMaxUniverse + 1, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err.find("universe") != std::string::npos);
    CHECK(plan(nullptr, nullptr, 5, 0, -1, -1, -1, nullptr) == ST_ERR_ARG && err == "permutations < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, 3, -1, -1, nullptr) == ST_ERR_ARG && err == "chunk_tasks < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, 3, -1, 0, nullptr) == ST_ERR_ARG && err == "stream < 0");
    CHECK(plan(nullptr, nullptr, 5, 0, (int64_t)1 << 31, 0, 0, nullptr) == ST_ERR_ARG && err.find("permutations") != std::string::npos);
    CHECK(plan(nullptr, nullptr, 5, 0, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "0 classes: 1 to 64");
    CHECK(plan(nullptr, nullptr, 5, 65, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "65 classes: 1 to 64");
    CHECK(plan(nullptr, c, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "y or cls is NULL");
    CHECK(plan(y, nullptr, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "y or cls is NULL");
    CHECK(plan(y, c, 5, 3, 3, 0, 0, nullptr) == ST_ERR_ARG && err == "out is NULL");
    uint8_t bad[10] = {0, 1, 255, 1, 2, 254, 1, 0, 0, 1};
    CHECK(plan(y, bad, 5, 2, 2, 0, 0, out) == ST_ERR_ARG && err == "cls[4] = 2 of 2 classes");
    CHECK(plan(y, bad, 5, 3, 2, 0, 0, out) == ST_ERR_ARG && err == "cls[5] = 254 of 3 classes");
    CHECK(plan(y, c, 5, 3, 2, 0, 0, out, 0) == ST_ERR_ARG && plan(y, c, 5, 3, 2, 0, 0, out, kClassSliceMax + 1) == ST_ERR_ARG);
    CHECK(plan(y, c, 5, 3, 2, 0, 0, out) == ST_OK);
    return 0;
}

int main()
{
    for (int32_t n : {3, 4, 5, 64, 65, 257})
        for (int32_t K : {1, 2, 6, 64}) {
            const Case C = make_case(n, K, 0);
            const int64_t perms = n > 100 ? 2 : 5;
            if (check_case(C, perms, 0, kClassSlice, rnd(), (int32_t)(rnd() % 1000))) return 1;
            for (int32_t slice : {1, 3, kClassSlice, kClassSliceMax})
                for (int64_t chunk : {1, 2, 5, 40})
                    if (n < 100 && K == 6 && check_case(C, 7, chunk, slice, rnd(), 0)) return 1;
        }
    if (check_case(make_case(257, 1, 1), 2, 16, 3, 11, 0) || check_case(make_case(257, 2, -1), 2, 0, 16, 12, 0)) return 1;
    // the bound of a block's partial sums cuts the blocks before the bound of the sigma rows does: 1025 row pairs x 64 classes
    {
        std::string err;
        ClassPlan P;
        int64_t out = 0;
        const Case C = make_case(2049, 64, 0);
        CHECK(class_plan(C.y.data(), C.cls.data(), 2049, 64, 999, 0, 0, kClassSlice, &out, P, err) == ST_OK);
        CHECK(P.perm_block == std::min<int64_t>(kClassPartBytes / (8 * 64 * 1025), 1000) && P.perm_block * 1025 * 64 * 8 <= kClassPartBytes);
    }
    if (check_blocks() || check_rows() || check_errors()) return 1;
    std::printf("sanitize class ok\n");
    return 0;
}
