// plan_checks.h -- what the host-only plan units (*_plan.cpp) share in their argument checks, plain C++17: how a check
// fails, and the check of a table of position sets (dispersion_plan, unifrac_plan).  Header-only.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/suchtree_hip.h"

namespace st {

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

}  // namespace st
