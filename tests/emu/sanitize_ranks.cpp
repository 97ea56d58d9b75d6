// The host side of the exact Spearman rank sums (suchtree_amd/csrc/rank_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_spearman_host.py builds this with -fsanitize=address,undefined): the key transform, the slot layout,
// the tie arithmetic and spearman_host against a direct O(n^2) count of "less" and "equal".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/rank_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static i128 sxy_of(const st_rank_sums &r) { return (i128)(((u128)(uint64_t)r.sxy_hi << 64) | r.sxy_lo); }
static u128 wide(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }

// a of every value by counting, O(n^2)
static std::vector<int64_t> centered(const std::vector<float> &v)
{
    const int64_t n = (int64_t)v.size();
    std::vector<int64_t> a(n);
    for (int64_t i = 0; i < n; i++) {
        int64_t less = 0, equal = 0;
        for (int64_t j = 0; j < n; j++) {
            less += v[j] < v[i];
            equal += v[j] == v[i];
        }
        a[i] = 2 * less + equal - n;
    }
    return a;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // keys keep the order of the values; the two zeros share one key
    const float ordered[] = {-inf, -3.0e38f, -1.5f, -1.0e-40f, 0.0f, 1.0e-45f, 1.0e-40f, 1.0f, 3.0e38f, inf};
    for (size_t i = 0; i + 1 < sizeof ordered / sizeof *ordered; i++) CHECK(rank_key(bits_of(ordered[i])) < rank_key(bits_of(ordered[i + 1])));
    CHECK(rank_key(bits_of(-0.0f)) == rank_key(bits_of(0.0f)));
    CHECK(rank_is_nan(bits_of(nan)) && rank_is_nan(bits_of(-nan)) && !rank_is_nan(bits_of(inf)) && !rank_is_nan(bits_of(-inf)));
    CHECK(rank_key(bits_of(-inf)) >> kRankLowBits < (uint32_t)kRankBuckets && rank_key(bits_of(inf)) >> kRankLowBits == 0xFF8u);

    // slots: the occupied buckets in order, every index inside its table
    std::vector<uint32_t> occ(kRankBuckets, 0u);
    occ[0] = 7, occ[17] = 1, occ[kRankBuckets - 1] = 3;
    RankSlots S;
    rank_slots(occ.data(), S);
    CHECK(S.n_slots == 3 && S.slot[0] == 0 && S.slot[17] == 1 && S.slot[kRankBuckets - 1] == 2 && S.slot[1] == -1);
    CHECK(rank_table_index(2, 0xFFFFFFFFu) == 3 * kRankBucketKeys - 1 && rank_table_index(0, 0x00100000u) == 0);

    // the largest case of the tie arithmetic: n = 2^31 - 1 values, all distinct / all equal
    {
        const uint64_t n = (uint64_t)kRankMaxPairs;
        st_rank_sums r;
        rank_finish((int64_t)n, 0, (int64_t)n, 1, 0, 0, rank_tie_term(n), &r);
        CHECK(wide(r.sxx_lo, r.sxx_hi) == ((u128)n * n * n - n) / 3 && r.syy_lo == 0 && r.syy_hi == 0);
        CHECK(rank_centered((int64_t)n - 1, 1, (int64_t)n) == (int32_t)(n - 1) && rank_centered(0, 1, (int64_t)n) == -(int32_t)(n - 1));
        rank_finish(5, 0, 1, 1, -(i128)7, 0, 0, &r);
        CHECK(r.sxy_hi == -1 && r.sxy_lo == (uint64_t)-7 && sxy_of(r) == -7);
    }

    std::string err;
    st_rank_sums r;
    std::mt19937 rng(5);
    for (int round = 0; round < 6; round++) {
        const int n = round == 0 ? 1 : round == 1 ? 2 : 700 + 37 * round;
        std::vector<float> x(n), y(n);
        for (int i = 0; i < n; i++) {
            x[i] = (float)((int)(rng() % 41) - 20) * (round % 2 ? 0.25f : 1.0e-41f);      // heavy ties; subnormals on even rounds
            if (rng() % 50 == 0) x[i] = rng() % 2 ? inf : -0.0f;
            y[i] = round == 5 ? -x[i] : x[i] * 0.5f + (float)(rng() % 7);
        }
        CHECK(spearman_host(x.data(), y.data(), n, &r, err) == ST_OK);
        const std::vector<int64_t> a = centered(x), b = centered(y);
        i128 sxy = 0, sxx = 0, syy = 0;
        for (int i = 0; i < n; i++) {
            sxy += (i128)a[i] * b[i];
            sxx += (i128)a[i] * a[i];
            syy += (i128)b[i] * b[i];
        }
        CHECK(r.n == n && r.n_nan == 0 && sxy_of(r) == sxy && wide(r.sxx_lo, r.sxx_hi) == (u128)sxx && wide(r.syy_lo, r.syy_hi) == (u128)syy);
        if (round == 5) CHECK(sxy == -sxx);
    }
    // NaN, empty, errors
    {
        const float x[] = {1.0f, nan, 3.0f}, y[] = {2.0f, 1.0f, nan};
        CHECK(spearman_host(x, y, 3, &r, err) == ST_OK && r.n == 3 && r.n_nan == 2 && r.sxx_lo == 0 && r.distinct_x == 0);
        CHECK(spearman_host(nullptr, nullptr, 0, &r, err) == ST_OK && r.n == 0 && r.sxy_lo == 0);
        CHECK(spearman_host(x, y, -1, &r, err) == ST_ERR_ARG);
        CHECK(spearman_host(x, nullptr, 3, &r, err) == ST_ERR_ARG);
        CHECK(spearman_host(x, y, 3, nullptr, err) == ST_ERR_ARG);
        CHECK(spearman_host(x, y, (int64_t)kRankMaxPairs + 1, &r, err) == ST_ERR_ARG && !err.empty());
    }
    std::printf("sanitize ranks ok\n");
    return 0;
}
