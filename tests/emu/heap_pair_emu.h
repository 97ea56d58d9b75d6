// heap_pair_emu.h -- TEST INFRASTRUCTURE ONLY.
//
// The pair function of the heap-family kernels (suchtree_amd/csrc/kernels_canopy_heap.h: heap_pairs) on the host, one pair at
// a time with the heap image as a plain array: leaf slots, the climb count k, the MRCA id by arithmetic, six line values and
// max(k - 6, 0) heap entries per side, every add predicated with -0.0f from a sum that starts at +0.0f; pairs with an
// internal node are walked on the tree (pair_math.h: pair_walk), as the kernels do.  What differs between the two kernels
// is how the six line values of a leaf slot are found: the caller's `six`.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../suchtree_amd/csrc/pair_math.h"
#include "../../suchtree_amd/csrc/tree_prep.h"

static inline float add_if(float s, bool on, float e)
{
    const uint32_t pad_bits = 0x80000000u;      // -0.0f: the identity of a float add
    float pad;
    std::memcpy(&pad, &pad_bits, 4);
    volatile float r = s + (on ? e : pad);
    return r;
}

// six(slot, e): e[0 .. 5] = the six lowest edges of the slot's lineage, false (with err set) when a load was refused.
// Returns 0, 3 on an id out of range, 4 on a refused load.
template <typename Six>
static int heap_pairs_emu(const st::TreeTables &T, int64_t n_nodes, const int64_t *pairs, int64_t n, double *out_d, int32_t *out_m,
                          std::string &err, Six six)
{
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) { err = "id out of range"; return 3; }
        if ((a | b) & 1) {
            const st::PairResult r = st::pair_walk(T.nodes.data(), T.depth.data(), T.stride.data(), (int32_t)a, (int32_t)b);
            out_d[i] = (double)r.dist;
            out_m[i] = r.mrca;
            continue;
        }
        const uint32_t sa = (uint32_t)a >> 1, sb = (uint32_t)b >> 1, x = sa ^ sb;
        int k = 0;
        while (k < 32 && (x >> k)) k++;
        float s = 0.0f;
        for (const uint32_t sl : {sa, sb}) {
            float e[6];
            if (!six(sl, e)) return 4;
            for (int j = 0; j < 6; j++) s = add_if(s, j < k, e[j]);
            uint32_t u = (1u << (T.heap_levels - 6)) + (sl >> 6);
            for (int q = 6; q < k; q++) {
                s = add_if(s, true, T.heap_dist[u]);
                u >>= 1;
            }
        }
        out_d[i] = (double)s;
        out_m[i] = k ? (int32_t)((((((sa >> k) << 1) | 1u) << k)) - 1u) : (int32_t)a;
    }
    return 0;
}
