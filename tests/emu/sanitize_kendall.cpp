// The host side of the exact Kendall counts (suchtree_amd/csrc/kendall_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_kendall_host.py builds this with -fsanitize=address,undefined): the key, the run bounds, the merge path
// and the lane merge at their edges, and kendall_host / kendall_host_tiled against a direct O(n^2) count.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/kendall_plan.h"

using namespace st;

#define CHECK(...)                                                               \
    do {                                                                         \
        if (!(__VA_ARGS__)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static st_kendall_counts brute(const std::vector<float> &x, const std::vector<float> &y)
{
    st_kendall_counts c{(int64_t)x.size(), 0, 0, 0, 0, 0};
    for (size_t i = 0; i < x.size(); i++)
        for (size_t j = i + 1; j < x.size(); j++) {
            const int sx = (x[j] > x[i]) - (x[j] < x[i]), sy = (y[j] > y[i]) - (y[j] < y[i]);
            c.discordant += sx * sy < 0;
            c.ties_x += sx == 0;
            c.ties_y += sy == 0;
            c.ties_xy += sx == 0 && sy == 0;
        }
    return c;
}

static bool same(const st_kendall_counts &a, const st_kendall_counts &b)
{
    return a.n == b.n && a.n_nan == b.n_nan && a.discordant == b.discordant && a.ties_x == b.ties_x && a.ties_y == b.ties_y &&
           a.ties_xy == b.ties_xy;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the key orders by x, then y; the two zeros share one key; no key is the padding key
    CHECK(kendall_key(bits_of(1.0f), bits_of(inf)) < kendall_key(bits_of(1.5f), bits_of(-inf)));
    CHECK(kendall_key(bits_of(1.0f), bits_of(-2.0f)) < kendall_key(bits_of(1.0f), bits_of(-1.0f)));
    CHECK(kendall_key(bits_of(-0.0f), bits_of(0.0f)) == kendall_key(bits_of(0.0f), bits_of(-0.0f)));
    CHECK(kendall_key(bits_of(inf), bits_of(inf)) < ~(uint64_t)0 && rank_key(bits_of(inf)) < ~(uint32_t)0);

    // run bounds: a whole pair, a short left run without a partner, a short right run, the largest call
    {
        KendallRun R = kendall_run(5, 4, 100);
        CHECK(R.left == 0 && R.mid == 4 && R.end == 8);
        R = kendall_run(97, 8, 100);
        CHECK(R.left == 96 && R.mid == 100 && R.end == 100);
        R = kendall_run(90, 8, 93);
        CHECK(R.left == 80 && R.mid == 88 && R.end == 93);
        const int64_t n = kRankMaxPairs, run = (int64_t)ST_KENDALL_TILE << 19;      // the last level of the largest call
        R = kendall_run(n - 1, run, n);
        CHECK(R.left == 0 && R.mid == run && R.end == n);
        R = kendall_run(n - 1, run >> 1, n);
        CHECK(R.left == run && R.mid == run + (run >> 1) && R.end == n);
    }
    // merge path and lane merge: equal keys go left first and close no inversion
    {
        const uint32_t a[] = {1, 3, 3, 7}, b[] = {0, 3, 3, 8, 9};
        const uint32_t want[] = {0, 1, 3, 3, 3, 3, 7, 8, 9};
        const int from_a[] = {0, 0, 1, 2, 3, 3, 3, 4, 4, 4};
        for (int d = 0; d <= 9; d++) CHECK(kendall_merge_path<int, uint32_t>(a, 4, b, 5, d) == from_a[d]);
        CHECK(kendall_merge_path<int, uint32_t>(a, 4, b, 0, 3) == 3 && kendall_merge_path<int, uint32_t>(a, 0, b, 5, 3) == 0);
        uint64_t inv = 0;
        std::vector<uint32_t> out(9);
        for (int d = 0; d < 9; d += 2) inv += kendall_lane_merge<true, int, uint32_t>(a, 4, b, 5, d, std::min(2, 9 - d), out.data() + d, 4);
        CHECK(std::equal(out.begin(), out.end(), want) && inv == 4 + 1 + 1);      // 0 passes four keys, each 3 of b passes the 7
        uint32_t k[kKendallLaneKeys] = {5, 5, 1, 9, 0, 5, 2, 9};
        CHECK((kendall_lane_sort<true, uint32_t>(k)) == 3 + 3 + 1 + 3 + 0 + 1 && std::is_sorted(k, k + kKendallLaneKeys));
        CHECK(kendall_tie_term(1) == 0 && kendall_tie_term(4) == 6 && kendall_tie_term((uint64_t)kRankMaxPairs) == 2305843005992468481ull);
    }

    std::string err;
    st_kendall_counts r, t;
    std::mt19937 rng(5);
    for (int round = 0; round < 8; round++) {
        const int n = round < 3 ? round : 500 + 61 * round;
        std::vector<float> x(n), y(n);
        for (int i = 0; i < n; i++) {
            x[i] = (float)((int)(rng() % 9) - 4) * (round % 2 ? 0.25f : 1.0e-41f);      // heavy ties; subnormals on even rounds
            if (rng() % 40 == 0) x[i] = rng() % 2 ? inf : -0.0f;
            y[i] = round == 5 ? -x[i] : round == 6 ? x[i] : x[i] * 0.5f + (float)(rng() % 3);
        }
        CHECK(kendall_host(x.data(), y.data(), n, &r, err) == ST_OK);
        CHECK(same(r, brute(x, y)));
        if (round == 5 && n > 1) CHECK(r.ties_x == r.ties_y && r.ties_x == r.ties_xy && r.discordant == (uint64_t)n * (n - 1) / 2 - r.ties_x);
        if (round == 6) CHECK(r.discordant == 0 && r.ties_x == r.ties_xy);
        for (int64_t tile : {1, 3, 4, 8, 24, 64, 1000}) {
            CHECK(kendall_host_tiled(x.data(), y.data(), n, tile, &t, err) == ST_OK);
            CHECK(same(r, t));
        }
    }
    // NaN, empty, errors
    {
        const float x[] = {1.0f, nan, 3.0f}, y[] = {2.0f, 1.0f, nan};
        CHECK(kendall_host(x, y, 3, &r, err) == ST_OK && r.n == 3 && r.n_nan == 2 && r.discordant == 0 && r.ties_x == 0);
        CHECK(kendall_host_tiled(x, y, 3, 4, &t, err) == ST_OK && same(r, t));
        CHECK(kendall_host(nullptr, nullptr, 0, &r, err) == ST_OK && r.n == 0 && r.ties_xy == 0);
        CHECK(kendall_host(x, y, -1, &r, err) == ST_ERR_ARG);
        CHECK(kendall_host(x, nullptr, 3, &r, err) == ST_ERR_ARG);
        CHECK(kendall_host(x, y, 3, nullptr, err) == ST_ERR_ARG);
        CHECK(kendall_host_tiled(x, y, 3, 0, &r, err) == ST_ERR_ARG);
        CHECK(kendall_host(x, y, (int64_t)kRankMaxPairs + 1, &r, err) == ST_ERR_ARG && !err.empty());
    }
    std::printf("sanitize kendall ok\n");
    return 0;
}
