// The host side of the exact linkage (suchtree_amd/csrc/linkage_plan.cpp) under AddressSanitizer + UBSan
// (tests/test_linkage_host.py builds this with -fsanitize=address,undefined): the cached chain against a plain scan of
// every active pair per step -- the definition of include/suchtree_hip.h written out once more, with __int128 -- over
// small and odd shapes, the three methods, tie-free codes at the top of the range, tie-heavy codes, all codes equal,
// weights, the case whose sums reach 60 bits and whose cross products reach 89, and every argument error in the stated
// order.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/linkage_plan.h"

using namespace st;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t g_state = 3232;
static uint64_t rnd() { return g_state = quartet_mix(g_state + 0x9E3779B97F4A7C15ull); }

// the definition: a scan of every active pair a < b per step, the first of least value stays
static std::vector<st_linkage_row> naive(const std::vector<int32_t> &codes, int32_t n, const int32_t *weights, int32_t method)
{
    const size_t N = (size_t)n;
    std::vector<__int128> S(N * N, 0);
    std::vector<long long> size(N), id(N);
    for (size_t i = 0; i < N; i++) {
        size[i] = weights ? weights[i] : 1;
        id[i] = (long long)i;
    }
    for (size_t i = 1; i < N; i++)
        for (size_t j = 0; j < i; j++)
            S[i * N + j] = S[j * N + i] = (__int128)codes[i * (i - 1) / 2 + j] * (method == ST_LINKAGE_AVERAGE ? size[i] * size[j] : 1);
    std::vector<st_linkage_row> rows;
    for (int32_t t = 0; t < n - 1; t++) {
        size_t ba = N, bb = N;
        __int128 bn = 0, bd = 1;
        for (size_t a = 0; a < N; a++)
            for (size_t b = a + 1; b < N; b++) {
                if (!size[a] || !size[b]) continue;
                const __int128 num = S[a * N + b], den = method == ST_LINKAGE_AVERAGE ? size[a] * size[b] : 1;
                if (ba == N || num * bd < bn * den) {
                    ba = a, bb = b, bn = num, bd = den;
                }
            }
        rows.push_back(st_linkage_row{(int64_t)bn, (int64_t)bd, (int32_t)std::min(id[ba], id[bb]), (int32_t)std::max(id[ba], id[bb]), size[ba] + size[bb]});
        for (size_t k = 0; k < N; k++) {
            if (!size[k] || k == ba || k == bb) continue;
            const __int128 va = S[k * N + ba], vb = S[k * N + bb];
            S[k * N + ba] = S[ba * N + k] = method == ST_LINKAGE_AVERAGE ? va + vb : method == ST_LINKAGE_SINGLE ? std::min(va, vb) : std::max(va, vb);
        }
        size[ba] += size[bb];
        size[bb] = 0;
        id[ba] = n + t;
    }
    return rows;
}

static int check_case(const std::vector<int32_t> &codes, int32_t n, const int32_t *weights)
{
    for (int32_t method : {ST_LINKAGE_AVERAGE, ST_LINKAGE_SINGLE, ST_LINKAGE_COMPLETE}) {
        std::string err;
        std::vector<st_linkage_row> got((size_t)n - 1);
        CHECK(linkage_args(codes.data(), n, weights, method, got.data(), err) == ST_OK);
        int64_t rescans = -1;
        linkage_host(codes.data(), n, weights, method, got.data(), &rescans);
        const std::vector<st_linkage_row> want = naive(codes, n, weights, method);
        CHECK(rescans >= n - 1);      // (row a at every step)
        for (int32_t t = 0; t < n - 1; t++) {
            const st_linkage_row &g = got[(size_t)t], &w = want[(size_t)t];
            CHECK(g.num == w.num && g.den == w.den && g.left == w.left && g.right == w.right && g.size == w.size);
            CHECK(g.left < g.right && g.right < n + t);
            if (t) CHECK((__int128)got[(size_t)t - 1].num * g.den <= (__int128)g.num * got[(size_t)t - 1].den);      // (reducible: monotone)
        }
        CHECK(got[(size_t)n - 2].size == [&] { int64_t s = 0; for (int32_t i = 0; i < n; i++) s += weights ? weights[i] : 1; return s; }());
    }
    return 0;
}

static std::vector<int32_t> random_codes(int32_t n, uint32_t lo, uint32_t span)
{
    std::vector<int32_t> c((size_t)n * (size_t)(n - 1) / 2);
    for (auto &v : c) v = (int32_t)(lo + (uint32_t)(rnd() >> 33) % span);
    return c;
}

int main()
{
    for (int32_t n : {2, 3, 4, 5, 33, 64, 65, 90}) {
        if (check_case(random_codes(n, 1u << 30, 1u << 30), n, nullptr)) return 1;      // the top of the range: tie-free but by chance
        if (check_case(random_codes(n, 1, 3), n, nullptr)) return 1;                    // {1, 2, 3}: ties at every step
        if (check_case(random_codes(n, 0, 2), n, nullptr)) return 1;                    // zeros among them
        if (check_case(std::vector<int32_t>((size_t)n * (size_t)(n - 1) / 2, 7), n, nullptr)) return 1;
        std::vector<int32_t> w((size_t)n);
        for (auto &v : w) v = 1 + (int32_t)(rnd() % 700);
        if (check_case(random_codes(n, 1u << 30, 1u << 30), n, w.data())) return 1;
        if (check_case(random_codes(n, 1, 3), n, w.data())) return 1;
    }
    {      // all codes equal at n = 17: (0, 1), (2, 17), (3, 18), ...
        const int32_t n = 17;
        std::vector<int32_t> c((size_t)n * (n - 1) / 2, 9);
        std::vector<st_linkage_row> got((size_t)n - 1);
        linkage_host(c.data(), n, nullptr, ST_LINKAGE_AVERAGE, got.data());
        CHECK(got[0].left == 0 && got[0].right == 1);
        for (int32_t t = 1; t < n - 1; t++) CHECK(got[(size_t)t].left == t + 1 && got[(size_t)t].right == n + t - 1 && got[(size_t)t].num == 9 * got[(size_t)t].den);
    }
    {      // sums of 60 bits, cross products of 89: what a 64-bit comparison gets wrong
        const int32_t n = 8;
        std::vector<int32_t> c, w((size_t)n, 8192);
        for (int32_t k = 0; k < n * (n - 1) / 2; k++) c.push_back(INT32_MAX - k);
        if (check_case(c, n, w.data())) return 1;
        std::vector<st_linkage_row> got((size_t)n - 1);
        linkage_host(c.data(), n, w.data(), ST_LINKAGE_AVERAGE, got.data());
        CHECK(got[(size_t)n - 2].num >> 59 && got[(size_t)n - 2].size == 65536);
    }
    {      // the argument checks, in the stated order
        std::string err;
        std::vector<int32_t> c = random_codes(5, 1, 100), w = {1, 2, 3, 4, 5};
        std::vector<st_linkage_row> out(4);
        CHECK(linkage_args(c.data(), 1, nullptr, 9, nullptr, err) == ST_ERR_ARG && err.find("n = 1 objects") == 0);
        CHECK(linkage_args(c.data(), kLinkageMaxObjects + 1, nullptr, 9, nullptr, err) == ST_ERR_ARG && err.find("n = 16385") == 0);
        CHECK(linkage_args(nullptr, 5, nullptr, 3, nullptr, err) == ST_ERR_ARG && err.find("method 3") == 0);
        CHECK(linkage_args(nullptr, 5, nullptr, 0, out.data(), err) == ST_ERR_ARG && err.find("NULL") != std::string::npos);
        CHECK(linkage_args(c.data(), 5, nullptr, 0, nullptr, err) == ST_ERR_ARG && err.find("NULL") != std::string::npos);
        c[7] = -4;
        w[2] = 0;
        CHECK(linkage_args(c.data(), 5, w.data(), 0, out.data(), err) == ST_ERR_ARG && err == "codes[7] = -4 is negative");
        c[7] = 4;
        CHECK(linkage_args(c.data(), 5, w.data(), 0, out.data(), err) == ST_ERR_ARG && err == "weights[2] = 0: at least 1");
        w[2] = 65536 - 11;
        CHECK(linkage_args(c.data(), 5, w.data(), 0, out.data(), err) == ST_ERR_ARG && err == "a total weight of 65537: at most 65536");
        w[2] = 65536 - 12;
        CHECK(linkage_args(c.data(), 5, w.data(), 2, out.data(), err) == ST_OK);
    }
    CHECK(linkage_row_stride(1) == 32 && linkage_row_stride(32) == 32 && linkage_row_stride(33) == 96 && linkage_row_stride(64) == 96);
    CHECK(linkage_row_stride(16384) == 16416 && (linkage_row_stride(4096) / 32) % 2 == 1);
    std::printf("sanitize linkage ok\n");
    return 0;
}
