// linkage_plan.h -- the host-only side of exact agglomerative clustering (st_linkage_codes: compare.linkage), plain C++17.
// No GPU calls in here (linkage_plan.cpp): the "not gpu" tests run it under the address / undefined-behaviour sanitizers
// (tests/emu/sanitize_linkage.cpp).  The definitions are the contract of include/suchtree_hip.h (st_linkage_codes); what
// the kernels share with the restatement -- the candidate, its order, the update of a pair sum -- is here too
// (kernels_linkage.h).
//
// The cache.  Slot k keeps its nearest later partner: the active b > k of least value S(k, b) / (s_k s_b), the least b on a
// tie (kLinkageNone when no later slot is active).  The pair of a step is then the row of least cached value, the least
// row on a tie, with its partner: least value, least a, least b.  After the merge of a < b into a, with S(k, a) updated for
// every active k:
//   - rows k < a whose partner was a or b, rows a < k < b whose partner was b, and row a are scanned again;
//   - every other row k < a compares the new S(k, a) with its entry, and takes a on a lower value or on an equal one when
//     a is below its partner (reducibility: the new value is never below the entry's);
//   - no other row has a pair that changed.
#pragma once
#include <cstdint>
#include <string>

#include "plan_checks.h"

namespace st {

constexpr int32_t kLinkageMaxObjects = ST_LINKAGE_MAX_OBJECTS;
constexpr int64_t kLinkageMaxWeight = ST_LINKAGE_MAX_WEIGHT;
constexpr int kLinkageNone = INT32_MAX;      // the key of no candidate
constexpr int kLinkageExpandThreads = 256;   // the two grid passes
constexpr int kLinkageChainThreads = 1024;   // the one workgroup of the chain: 16 waves, 4 per SIMD
// the chain's cache in LDS: 8 (value) + 4 (partner) + 4 (size) bytes per slot, 128 KiB here, beside 768 bytes of partials
constexpr int32_t kLinkageLdsMaxObjects = 8192;

// The device's row stride of S in elements: n rounded up to 256 bytes, then an odd number of such units.  The chain
// writes column a once per step, one element per row: with a stride of a power of two those writes would all fall
// on one memory channel.
constexpr uint32_t linkage_row_stride(int32_t n) { return (((uint32_t)n + 31u) & ~31u) | 32u; }

// A candidate: the value num / den and the index that breaks a tie (the row in the arg-min over rows, the partner in
// the scan of a row); aux rides along (the row's partner in the arg-min).
struct LinkageCand {
    long long num, den;
    int key, aux;
};

ST_QUARTET_HD LinkageCand linkage_none() { return LinkageCand{0, 1, kLinkageNone, 0}; }

// x before y: the lower value, by cross-multiplication in 128 bits (num < 2^62, den <= 2^30), then the lower key
ST_QUARTET_HD bool linkage_before(const LinkageCand &x, const LinkageCand &y)
{
    if (x.key == kLinkageNone) return false;
    if (y.key == kLinkageNone) return true;
    const unsigned __int128 l = (unsigned __int128)(unsigned long long)x.num * (unsigned long long)y.den;
    const unsigned __int128 r = (unsigned __int128)(unsigned long long)y.num * (unsigned long long)x.den;
    return l < r || (l == r && x.key < y.key);
}

// S(k, a) after b joined a
ST_QUARTET_HD long long linkage_merge(int method, long long va, long long vb)
{
    return method == ST_LINKAGE_AVERAGE ? va + vb : method == ST_LINKAGE_SINGLE ? (va < vb ? va : vb) : (va > vb ? va : vb);
}

// the denominator of the pair of two slots of these sizes
ST_QUARTET_HD long long linkage_den(int method, long long s_a, long long s_b) { return method == ST_LINKAGE_AVERAGE ? s_a * s_b : 1; }

// ST_OK, or ST_ERR_ARG with `err`: the checks of st_linkage_codes, in its order
int linkage_args(const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, const st_linkage_row *out, std::string &err);

// the chain on the host, with the cache above; rescans (may be NULL) gets the rows scanned again over all steps, row a's
// included
void linkage_host(const int32_t *codes, int32_t n, const int32_t *weights, int32_t method, st_linkage_row *out, int64_t *rescans = nullptr);

}  // namespace st
