// quartet_plan.cpp -- see quartet_plan.h.  Integer arithmetic over caller-supplied arrays: no GPU calls.
#include "quartet_plan.h"

namespace st {

int64_t quartet_total(int64_t m) { return m < 4 ? 0 : (int64_t)quartet_choose4((uint64_t)m); }

int quartet_range_args(int mode, int64_t m, int64_t k_begin, int64_t k_count, std::string &err)
{
    if (mode != ST_QUARTET_ALL && mode != ST_QUARTET_SAMPLE) {
        err = "mode must be ST_QUARTET_ALL or ST_QUARTET_SAMPLE";
        return ST_ERR_ARG;
    }
    if (m < 0 || k_begin < 0 || k_count < 0) {
        err = "negative size";
        return ST_ERR_ARG;
    }
    if (mode == ST_QUARTET_ALL) {
        if (m > kQuartetMaxLeavesAll) {
            err = "all quartets of " + std::to_string(m) + " leaves: at most " + std::to_string(kQuartetMaxLeavesAll) + " leaves (sample instead)";
            return ST_ERR_ARG;
        }
        const int64_t total = quartet_total(m);
        if (k_begin > total || k_count > total - k_begin) {
            err = "quartet range exceeds C(m,4) = " + std::to_string(total);
            return ST_ERR_ARG;
        }
        return ST_OK;
    }
    if (m > kQuartetMaxLeavesSample) {
        err = "sampled quartets: m must be below 2^31";
        return ST_ERR_ARG;
    }
    if (m < 4 && k_count > 0) {
        err = "a quartet needs four leaves, m = " + std::to_string(m);
        return ST_ERR_ARG;
    }
    if (k_begin > kQuartetMaxSampleEnd || k_count > kQuartetMaxSampleEnd - k_begin) {
        err = "sampled quartets: k_begin + k_count must be at most 2^62";
        return ST_ERR_ARG;
    }
    return ST_OK;
}

int quartet_chunk_arg(int64_t chunk_quartets, std::string &err)
{
    if (chunk_quartets >= 0 && chunk_quartets <= kQuartetMaxChunk) return ST_OK;
    err = "chunk_quartets must be 0 or a positive value of at most " + std::to_string(kQuartetMaxChunk) + " (below 2^31 / 6)";
    return ST_ERR_ARG;
}

void quartet_positions_host(int mode, uint64_t seed, int64_t m, int64_t k_begin, int64_t k_count, int32_t *out_pos)
{
    for (int64_t i = 0; i < k_count; i++) {
        if (mode == ST_QUARTET_ALL) quartet_unrank((uint64_t)(k_begin + i), m, out_pos + 4 * i);
        else quartet_draw(seed, (uint64_t)(k_begin + i), m, out_pos + 4 * i, QuartetMulHiHost{});
    }
}

}  // namespace st
