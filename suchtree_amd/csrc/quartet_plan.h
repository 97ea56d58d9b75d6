// quartet_plan.h -- the host-only side of the quartet comparison (st_quartet_positions, st_compare_quartets_*_host),
// plain C++17, and the inline functions the device shares with it (kernels_quartets.h): which four positions quartet k
// of a leaf list is -- unranked from all C(m,4) subsets, or drawn from (seed, k, m) -- and the class of a quartet from
// its six MRCA ids.  No GPU calls in here (quartet_plan.cpp): the "not gpu" tests run it under the address /
// undefined-behaviour sanitizers.  The definitions are the contract of include/suchtree_hip.h (st_quartet_table).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/suchtree_hip.h"

#if defined(__HIP__)      // (spelled as attributes: hipcc compiles quartet_plan.cpp as HIP too, without the runtime header)
#define ST_QUARTET_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define ST_QUARTET_HD inline
#endif

namespace st {

constexpr int64_t kQuartetMaxLeavesAll = 65536;                      // C(65536, 4) < 2^60
constexpr int64_t kQuartetMaxLeavesSample = ((int64_t)1 << 31) - 1;    // positions are int32
constexpr int64_t kQuartetMaxSampleEnd = (int64_t)1 << 62;            // 4 k + 4 stays within 64 bits
constexpr int64_t kQuartetMaxChunk = (((int64_t)1 << 31) - 1) / 6;    // six MRCA ids per quartet, indexed within 2^31

// C(p, r) for the p the unranking meets (p <= 65536): every intermediate stays below 2^62
ST_QUARTET_HD uint64_t quartet_choose2(uint64_t p) { return p * (p - 1) / 2; }      // (p = 0: 0 * (2^64 - 1) / 2 = 0)
ST_QUARTET_HD uint64_t quartet_choose3(uint64_t p) { return p < 3 ? 0 : p * (p - 1) / 2 * (p - 2) / 3; }
ST_QUARTET_HD uint64_t quartet_choose4(uint64_t p) { return p < 4 ? 0 : quartet_choose2(p) * quartet_choose2(p - 2) / 6; }

// the largest p in [lo, hi] with C(p, r) <= k, from a guess: exact 64-bit comparisons, looped -- the floating-point
// root that made the guess may be off by more than one near 2^60
template <typename Choose>
ST_QUARTET_HD int64_t quartet_settle(int64_t p, int64_t lo, int64_t hi, uint64_t k, Choose choose)
{
    p = p < lo ? lo : p > hi ? hi : p;
    while (p > lo && choose((uint64_t)p) > k) p--;
    while (p < hi && choose((uint64_t)p + 1) <= k) p++;
    return p;
}

// ST_QUARTET_ALL: quartet k of m leaves, 0 <= k < C(m, 4), 4 <= m <= 65536, is the k-th 4-subset p0 < p1 < p2 < p3 of
// the positions in colexicographic order: p3 the largest p with C(p, 4) <= k, k -= C(p3, 4), p2 the largest p with
// C(p, 3) <= k, and so on down to p0.
ST_QUARTET_HD void quartet_unrank(uint64_t k, int64_t m, int32_t p[4])
{
    // C(p, 4) ~ (p - 1.5)^4 / 24, C(p, 3) ~ (p - 1)^3 / 6, C(p, 2) ~ (p - 0.5)^2 / 2
    const int64_t p3 = quartet_settle((int64_t)(sqrt(sqrt(24.0 * (double)k)) + 1.5), 3, m - 1, k,
                                      [](uint64_t q) { return quartet_choose4(q); });
    k -= quartet_choose4((uint64_t)p3);
    const int64_t p2 = quartet_settle((int64_t)(cbrt(6.0 * (double)k) + 1.0), 2, p3 - 1, k,
                                      [](uint64_t q) { return quartet_choose3(q); });
    k -= quartet_choose3((uint64_t)p2);
    const int64_t p1 = quartet_settle((int64_t)(sqrt(2.0 * (double)k) + 0.5), 1, p2 - 1, k,
                                      [](uint64_t q) { return quartet_choose2(q); });
    k -= quartet_choose2((uint64_t)p1);
    p[0] = (int32_t)k;
    p[1] = (int32_t)p1;
    p[2] = (int32_t)p2;
    p[3] = (int32_t)p3;
}

// the splitmix64 finalizer
ST_QUARTET_HD uint64_t quartet_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// high 64 bits of a 64 x 64 bit product on the host (the kernels pass __umul64hi: kernels_quartets.h)
struct QuartetMulHiHost {
    ST_QUARTET_HD uint64_t operator()(uint64_t a, uint64_t b) const { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
};

// ST_QUARTET_SAMPLE: quartet k of m leaves, 4 <= m < 2^31, depends on (seed, k, m) alone.  Draw j = 0..3 is
// r_j = high 64 bits of mix(seed + (4 k + j + 1) * 0x9E3779B97F4A7C15) * (m - j), a rank among the positions not yet
// chosen: going through those already chosen in increasing order, p_j++ whenever p_j >= q.  The four positions are
// distinct, in draw order.  (`chosen` is kept sorted by compare-and-swap at fixed indices: registers on the device.)
template <typename MulHi>
ST_QUARTET_HD void quartet_draw(uint64_t seed, uint64_t k, int64_t m, int32_t p[4], MulHi mulhi)
{
    int64_t chosen[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t u = quartet_mix(seed + (4 * k + (uint64_t)j + 1) * 0x9E3779B97F4A7C15ull);
        int64_t v = (int64_t)mulhi(u, (uint64_t)(m - j));
#pragma unroll
        for (int i = 0; i < j; i++)
            if (v >= chosen[i]) v++;
        p[j] = (int32_t)v;
        chosen[j] = v;
#pragma unroll
        for (int i = j; i > 0; i--)
            if (chosen[i] < chosen[i - 1]) { const int64_t t = chosen[i]; chosen[i] = chosen[i - 1]; chosen[i - 1] = t; }
    }
}

template <int MODE, typename MulHi>
ST_QUARTET_HD void quartet_positions_of(uint64_t seed, uint64_t k, int64_t m, int32_t p[4], MulHi mulhi)
{
    if (MODE == ST_QUARTET_ALL) quartet_unrank(k, m, p);
    else quartet_draw(seed, k, m, p, mulhi);
}

// Class of a quartet (a,b,c,d) from its six MRCA ids in the reference's order ab ac ad bc bd cd: the first index whose
// id occurs exactly once among the six is the pick (SuchTree/MuchTree.pyx:1364-1372); 0 = ab|cd (pick 0 or 5),
// 1 = ac|bd (1 or 4), 2 = ad|bc (2 or 3), 3 = no id is unique (the reference then reports ab|cd) -- or an id is
// negative, which the checked ids of the compare path never produce.
ST_QUARTET_HD int quartet_class(const int32_t m[6])
{
    int pick = 6;
    bool bad = false;
    for (int j = 5; j >= 0; j--) {
        int c = 0;
        for (int k = 0; k < 6; k++) c += m[j] == m[k];
        if (c == 1) pick = j;
        bad |= m[j] < 0;
    }
    if (bad || pick == 6) return 3;
    return pick < 3 ? pick : 5 - pick;
}

// ---- host only (quartet_plan.cpp) ----
// C(m, 4) for 0 <= m <= 65536
int64_t quartet_total(int64_t m);
// ST_OK, or ST_ERR_ARG with `err`: the mode, m and the range [k_begin, k_begin + k_count) against the limits above
int quartet_range_args(int mode, int64_t m, int64_t k_begin, int64_t k_count, std::string &err);
// chunk_quartets: 0 or a positive value below 2^31 / 6
int quartet_chunk_arg(int64_t chunk_quartets, std::string &err);
// the (k_count, 4) positions of quartets [k_begin, k_begin + k_count) (arguments already checked)
void quartet_positions_host(int mode, uint64_t seed, int64_t m, int64_t k_begin, int64_t k_count, int32_t *out_pos);

}  // namespace st
