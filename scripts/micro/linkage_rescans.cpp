// linkage_rescans.cpp -- how many rows the nearest-partner cache of st_linkage_codes scans again per step
// (scripts/linkage_bench.py builds and runs it: g++ -O2 -std=c++17 -I include linkage_rescans.cpp linkage_plan.cpp).
// Reads n (n - 1) / 2 int32 codes from the file named on the command line, runs the host restatement for the method
// given (0 average, 1 single, 2 complete) and prints "n steps rescans".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../suchtree_amd/csrc/linkage_plan.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int n = std::atoi(argv[2]), method = std::atoi(argv[3]);
    if (n < 2 || n > st::kLinkageMaxObjects) return 2;
    std::vector<int32_t> codes((size_t)n * (n - 1) / 2);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(codes.data(), 4, codes.size(), f) != codes.size()) return 3;
    std::fclose(f);
    std::vector<st_linkage_row> rows((size_t)n - 1);
    std::string err;
    if (st::linkage_args(codes.data(), n, nullptr, method, rows.data(), err) != ST_OK) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 4;
    }
    int64_t rescans = 0;
    st::linkage_host(codes.data(), n, nullptr, method, rows.data(), &rescans);
    std::printf("%d %d %lld\n", n, n - 1, (long long)rescans);
    return 0;
}
