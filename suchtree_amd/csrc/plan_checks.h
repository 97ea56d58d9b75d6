// plan_checks.h -- what the host-only plan units (*_plan.cpp) share in their argument checks, plain C++17: how a check
// fails, the check of a table of position sets (dispersion_plan, setpair_plan, unifrac_plan, unifrac_null_plan), and the
// triangle of set pairs -- its index, which the kernels share (kernels_unifrac.h, kernels_unifrac_null.h), and the check
// of a range of it (setpair_plan, unifrac_plan, unifrac_null_plan).  Header-only.
#pragma once
#include <cstdint>
#include <string>

#include "quartet_plan.h"      // ST_QUARTET_HD, the public header

namespace st {

// floor(sqrt(x)): integers only
ST_QUARTET_HD uint64_t unifrac_isqrt(uint64_t x)
{
    uint64_t r = 0, bit = (uint64_t)1 << 62;
    while (bit > x) bit >>= 2;
    while (bit) {
        if (x >= r + bit) {
            x -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
        bit >>= 2;
    }
    return r;
}

// pair k of the triangle: k = i (i - 1) / 2 + j, 0 <= j < i.  8 k + 1 = (2 i - 1)^2 + 8 j lies in [(2 i - 1)^2, (2 i + 1)^2).
// The device meets k < 2^59 (at most 2^30 sets).  The host alone meets 2^61 <= k < 2^62 (setpair_plan: more than 2^31
// sets), where 8 k + 1 no longer fits: there i is r or r + 1 of r = floor(sqrt(2 k)), by i (i - 1) <= 2 k < i (i + 1).
ST_QUARTET_HD void unifrac_pair(int64_t k, int64_t &i, int64_t &j)
{
    i = (int64_t)((1 + unifrac_isqrt(8 * (uint64_t)k + 1)) >> 1);
#if !defined(__HIP_DEVICE_COMPILE__)
    if (k >> 61) {
        const uint64_t r = unifrac_isqrt(2 * (uint64_t)k);
        i = (int64_t)(r * (r + 1) <= 2 * (uint64_t)k ? r + 1 : r);
    }
#endif
    j = k - i * (i - 1) / 2;
}

inline int fail(int code, std::string &err, const std::string &msg)
{
    err = msg;
    return code;
}

// A table of n_sets sets of positions in a universe of n: set r is set_pos[sets[r] .. sets[r + 1]).  ST_OK, or ST_ERR_ARG
// with `err`.  Checks, in this order: no negative count, n_pos within int32, NULL arrays, then set by set its offsets
// (0 <= sets[r] <= sets[r + 1] <= n_pos) and its positions (inside the universe, strictly increasing).
inline int position_sets_args(int32_t n, const int32_t *set_pos, int64_t n_pos, const int64_t *sets, int64_t n_sets, std::string &err)
{
    if (n_pos < 0 || n_sets < 0) return fail(ST_ERR_ARG, err, "negative size");
    if (n_pos > INT32_MAX) return fail(ST_ERR_ARG, err, "more than 2^31 - 1 positions");
    if ((n_sets > 0 && !sets) || (n_pos > 0 && !set_pos)) return fail(ST_ERR_ARG, err, "set_pos or sets is NULL");
    for (int64_t r = 0; r < n_sets; r++) {
        const int64_t b = sets[r], e = sets[r + 1];
        if (b < 0 || e < b || e > n_pos)
            return fail(ST_ERR_ARG, err, "set " + std::to_string(r) + ": offsets [" + std::to_string(b) + ", " + std::to_string(e) + ") of " +
                                             std::to_string(n_pos) + " positions");
        for (int64_t i = b; i < e; i++) {
            if (set_pos[i] < 0 || set_pos[i] >= n) return fail(ST_ERR_ARG, err, "set " + std::to_string(r) + ": a position outside the universe");
            if (i > b && set_pos[i] <= set_pos[i - 1])
                return fail(ST_ERR_ARG, err, "set " + std::to_string(r) + ": positions must be strictly increasing");
        }
    }
    return ST_OK;
}

// the range [begin, begin + count) inside a triangle with `total` pairs: ST_OK, or ST_ERR_ARG with `err` (the caller has
// checked the signs)
inline int triangle_range_args(int64_t total, int64_t begin, int64_t count, std::string &err)
{
    if (begin > total || count > total - begin)
        return fail(ST_ERR_ARG, err, "pairs [" + std::to_string(begin) + ", +" + std::to_string(count) + ") of a triangle of " + std::to_string(total));
    return ST_OK;
}

}  // namespace st
