// The host side of the quartet comparison (suchtree_amd/csrc/quartet_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_quartets_host.py builds this with -fsanitize=address,undefined): unranking against a direct enumeration
// and at the edges of the 64-bit arithmetic, the draw against its definition, the class rule, the argument checks.
#include <algorithm>
#include <array>
#include <cstdio>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/quartet_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// C(p, r) by the multiplicative formula in 128 bits
static unsigned __int128 choose(uint64_t p, int r)
{
    if (p < (uint64_t)r) return 0;
    unsigned __int128 c = 1;
    for (int i = 0; i < r; i++) c = c * (p - i) / (i + 1);
    return c;
}

int main()
{
    // every 4-subset of 0..m-1, ordered by (p3, p2, p1, p0): the colexicographic order
    for (int m = 4; m <= 14; m++) {
        std::vector<std::array<int32_t, 4>> want;
        for (int d = 3; d < m; d++)
            for (int c = 2; c < d; c++)
                for (int b = 1; b < c; b++)
                    for (int a = 0; a < b; a++) want.push_back({a, b, c, d});
        CHECK((int64_t)want.size() == quartet_total(m));
        std::vector<int32_t> got(4 * want.size());
        quartet_positions_host(ST_QUARTET_ALL, 0, m, 0, (int64_t)want.size(), got.data());
        for (size_t k = 0; k < want.size(); k++)
            for (int j = 0; j < 4; j++) CHECK(got[4 * k + j] == want[k][j]);
    }
    // the binomials against 128-bit arithmetic, and the block edges k = C(p,4) - 1 and C(p,4)
    for (uint64_t p : {0ull, 1ull, 3ull, 4ull, 5ull, 1000ull, 46341ull, 65535ull, 65536ull}) {
        CHECK(quartet_choose4(p) == choose(p, 4) && quartet_choose3(p) == choose(p, 3) && quartet_choose2(p) == choose(p, 2));
        if (p < 4 || p >= 65536) continue;
        int32_t q[4];
        const uint64_t k = quartet_choose4(p);
        quartet_unrank(k, 65536, q);
        CHECK(q[0] == 0 && q[1] == 1 && q[2] == 2 && q[3] == (int32_t)p);
        if (k > 0) {
            quartet_unrank(k - 1, 65536, q);
            CHECK(q[0] == (int32_t)p - 4 && q[1] == (int32_t)p - 3 && q[2] == (int32_t)p - 2 && q[3] == (int32_t)p - 1);
        }
    }
    CHECK(quartet_total(65536) == (int64_t)choose(65536, 4) && quartet_total(65536) < ((int64_t)1 << 60) && quartet_total(3) == 0);
    {
        int32_t q[4];
        quartet_unrank((uint64_t)quartet_total(65536) - 1, 65536, q);
        CHECK(q[0] == 65532 && q[1] == 65533 && q[2] == 65534 && q[3] == 65535);
        // the settle loop from guesses that are far off, on both sides
        auto c4 = [](uint64_t p) { return quartet_choose4(p); };
        for (int64_t guess : {-5ll, 3ll, 700ll, 1000ll, 65535ll, 1ll << 40})
            CHECK(quartet_settle(guess, 3, 65535, quartet_choose4(1000) + 17, c4) == 1000);
    }
    // the draw: distinct, below m, a function of (seed, k, m) alone; m = 4 gives permutations
    for (uint64_t seed : {0ull, 1ull, ~0ull}) {
        for (int64_t m : {4ll, 5ll, 1000ll, (1ll << 31) - 1}) {
            std::vector<int32_t> a(4 * 3000), b(4 * 1000);
            quartet_positions_host(ST_QUARTET_SAMPLE, seed, m, 0, 3000, a.data());
            quartet_positions_host(ST_QUARTET_SAMPLE, seed, m, 2000, 1000, b.data());
            CHECK(std::equal(b.begin(), b.end(), a.begin() + 8000));
            for (int k = 0; k < 3000; k++) {
                std::array<int32_t, 4> s = {a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]};
                std::sort(s.begin(), s.end());
                CHECK(s[0] >= 0 && s[0] < s[1] && s[1] < s[2] && s[2] < s[3] && s[3] < m);
            }
        }
    }
    // a range that ends at 2^62
    {
        int32_t q[8];
        quartet_positions_host(ST_QUARTET_SAMPLE, ~0ull, 1000, kQuartetMaxSampleEnd - 2, 2, q);
        for (int j = 0; j < 8; j++) CHECK(q[j] >= 0 && q[j] < 1000);
    }
    // the class rule
    {
        const int32_t ab_cd[6] = {1, 5, 5, 5, 5, 3}, ac_bd[6] = {5, 1, 5, 5, 3, 5}, ad_bc[6] = {5, 5, 1, 3, 5, 5};
        const int32_t last[6] = {5, 5, 5, 5, 5, 3}, none[6] = {4, 4, 4, 4, 4, 4}, neg[6] = {1, 5, 5, 5, 5, -1}, bd[6] = {5, 7, 5, 5, 3, 5};
        CHECK(quartet_class(ab_cd) == 0 && quartet_class(ac_bd) == 1 && quartet_class(ad_bc) == 2 && quartet_class(last) == 0);
        CHECK(quartet_class(none) == 3 && quartet_class(neg) == 3 && quartet_class(bd) == 1);
    }
    // arguments
    {
        std::string err;
        CHECK(quartet_range_args(ST_QUARTET_ALL, 3, 0, 0, err) == ST_OK && quartet_range_args(ST_QUARTET_ALL, 3, 0, 1, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_SAMPLE, 3, 0, 0, err) == ST_OK && quartet_range_args(ST_QUARTET_SAMPLE, 3, 0, 1, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_ALL, 65536, quartet_total(65536) - 1, 1, err) == ST_OK);
        CHECK(quartet_range_args(ST_QUARTET_ALL, 65536, quartet_total(65536), 1, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_ALL, 65537, 0, 0, err) == ST_ERR_ARG && quartet_range_args(2, 10, 0, 1, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_ALL, 10, INT64_MAX, INT64_MAX, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_SAMPLE, (1ll << 31) - 1, kQuartetMaxSampleEnd - 5, 5, err) == ST_OK);
        CHECK(quartet_range_args(ST_QUARTET_SAMPLE, 1ll << 31, 0, 1, err) == ST_ERR_ARG);
        CHECK(quartet_range_args(ST_QUARTET_SAMPLE, 10, kQuartetMaxSampleEnd - 5, 6, err) == ST_ERR_ARG && !err.empty());
        CHECK(quartet_range_args(ST_QUARTET_SAMPLE, 10, INT64_MAX, INT64_MAX, err) == ST_ERR_ARG && quartet_range_args(ST_QUARTET_SAMPLE, 10, -1, 1, err) == ST_ERR_ARG);
        CHECK(quartet_chunk_arg(0, err) == ST_OK && quartet_chunk_arg(kQuartetMaxChunk, err) == ST_OK);
        CHECK(quartet_chunk_arg(kQuartetMaxChunk + 1, err) == ST_ERR_ARG && quartet_chunk_arg(-1, err) == ST_ERR_ARG);
    }
    std::printf("sanitize quartets ok\n");
    return 0;
}
