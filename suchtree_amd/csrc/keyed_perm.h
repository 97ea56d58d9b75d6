// keyed_perm.h -- the keyed permutation that defines every null in the project (st_hommola_permutation: the rows of
// st_hommola_clades_host, the sigma rows of st_partner_dispersion_host), plain C++17 for host and device, no GPU calls:
// the stream hash and the key, the universe limit, the size classes of the device sort (kernels_perm.h) with their thread
// counts and LDS bytes, the host form with its argument check (under ASan / UBSan in tests/emu/sanitize_hommola.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "quartet_plan.h"

namespace st {

constexpr int32_t kPermMaxUniverse = ST_HOMMOLA_MAX_UNIVERSE;      // positions travel as 16 bits, keys carry 16 bits of index
constexpr uint64_t kPermGolden = 0x9E3779B97F4A7C15ull;

// the key of (seed, node, permutation p >= 1, side): h1, then w_i of universe position i.  Sorting the w of a universe
// gives the permutation: sigma[j] = low 16 bits of the j-th smallest w (the w are distinct).
ST_QUARTET_HD uint64_t perm_stream(uint64_t seed, int32_t node, int64_t p, int side)
{
    const uint64_t h0 = quartet_mix(seed + ((uint64_t)(int64_t)node + 1) * kPermGolden);
    return quartet_mix(h0 + (2 * (uint64_t)p + (uint64_t)side) * kPermGolden);
}
ST_QUARTET_HD uint64_t perm_key(uint64_t h1, uint32_t i)
{
    return (quartet_mix(h1 + ((uint64_t)i + 1) * kPermGolden) & 0xFFFFFFFFFFFF0000ull) | (uint64_t)i;
}

enum PermSortClass { kPermSortWave = 0, kPermSortSmall = 1, kPermSortLarge = 2 };
constexpr int kPermWaveMax = 64;           // universes of up to 64 positions: one wave, keys in registers
constexpr int kPermSmallMax = 2048;        // up to 2048: 256 lanes and 16 KiB of LDS; beyond: 1024 lanes, up to 128 KiB
constexpr int kPermSmallThreads = 256, kPermLargeThreads = 1024;      // the workgroups of the two LDS forms
ST_QUARTET_HD int perm_sort_class(int n) { return n <= kPermWaveMax ? kPermSortWave : n <= kPermSmallMax ? kPermSortSmall : kPermSortLarge; }

// the LDS of one sort of n positions: 8-byte keys, n rounded up to a power of two, at least 128
inline size_t perm_lds_bytes(int n)
{
    size_t N = 128;
    while (N < (size_t)n) N <<= 1;
    return N * 8;
}

inline int perm_args(int32_t node, int64_t p, int side, int32_t n, std::string &err)
{
    if (n < 1 || n > kPermMaxUniverse) err = "a universe of " + std::to_string(n) + " positions: 1 to " + std::to_string(kPermMaxUniverse);
    else if (p < 0) err = "permutation index < 0";
    else if (side != 0 && side != 1) err = "side must be 0 (the clade tree) or 1 (the other tree)";
    else if (node < 0) err = "node < 0";
    else return ST_OK;
    return ST_ERR_ARG;
}

// the permutation of (seed, node, p, side) over n positions, 1 <= n <= kPermMaxUniverse; p = 0: the identity
inline void perm_host(uint64_t seed, int32_t node, int64_t p, int side, int32_t n, int32_t *out)
{
    for (int32_t i = 0; i < n; i++) out[i] = i;
    if (p == 0) return;
    const uint64_t h1 = perm_stream(seed, node, p, side);
    std::vector<uint64_t> w((size_t)n);
    for (int32_t i = 0; i < n; i++) w[(size_t)i] = perm_key(h1, (uint32_t)i);
    std::sort(w.begin(), w.end());
    for (int32_t j = 0; j < n; j++) out[j] = (int32_t)(w[(size_t)j] & 0xFFFF);
}

}  // namespace st
