// kendall_host_tiled and kendall_host (suchtree_amd/csrc/kendall_plan.cpp) behind two C functions, for
// tests/test_kendall_host.py: it builds this file with kendall_plan.cpp and rank_plan.cpp into a small shared library
// (plain g++, no sanitizer) and compares the two restatements at small tiles.
#include <string>

#include "../../suchtree_amd/csrc/kendall_plan.h"

extern "C" int kendall_tiled(const float *x, const float *y, int64_t n, int64_t tile, st_kendall_counts *out)
{
    std::string err;
    return st::kendall_host_tiled(x, y, n, tile, out, err);
}

extern "C" int kendall_plain(const float *x, const float *y, int64_t n, st_kendall_counts *out)
{
    std::string err;
    return st::kendall_host(x, y, n, out, err);
}
