// heap_emulator.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Runs the product's heap-line tables (suchtree_amd/csrc/tree_prep.cpp: prepare_heap_lines) and the pair function of
// k_canopy_ilp_heap over them on the host, one pair at a time with the heap image as a plain array: leaf slots, the
// climb count k, the MRCA id by arithmetic, six line values and max(k - 6, 0) heap entries per side, every add
// predicated with -0.0f from a sum that starts at +0.0f; pairs with an internal node are walked on the tree
// (pair_math.h: pair_walk), as the kernel does.  Never loaded by suchtree_amd.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../suchtree_amd/csrc/pair_math.h"
#include "../../suchtree_amd/csrc/tree_prep.h"

using namespace st;

extern "C" {

static std::string g_err;
const char *heap_emu_last_error() { return g_err.c_str(); }

// Returns 0 admitted, 1 bad tree, 2 refused.  sizes = {floats of heap_lines, floats of heap_dist, levels}.
int heap_emu_prepare(const int32_t *parent, const float *distance, int64_t n_nodes, int64_t *sizes)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return 1;
    const bool ok = prepare_heap_lines(T);
    sizes[0] = (int64_t)T.heap_lines.size();
    sizes[1] = (int64_t)T.heap_dist.size();
    sizes[2] = T.heap_levels;
    return ok ? 0 : 2;
}

static inline float add_if(float s, bool on, float e)
{
    const uint32_t pad_bits = 0x80000000u;      // -0.0f: the identity of a float add
    float pad;
    std::memcpy(&pad, &pad_bits, 4);
    volatile float r = s + (on ? e : pad);
    return r;
}

static float side(const float *lines, const float *heap, int levels, uint32_t sl, int k, float s)
{
    const float *line = lines + (size_t)(sl >> 4) * 32;
    const uint32_t t = sl & 15u;
    // (tree_prep.h: groups of four leaves at floats 7g .. 7g+6 -- own own h1 h2 h1 own own --, then e3 e4 e5 e3)
    const float *G = line + 7 * (t >> 2);
    const uint32_t r = t & 3u;
    s = add_if(s, 0 < k, G[r < 2 ? r : r + 3]);
    s = add_if(s, 1 < k, G[r < 2 ? 2 : 4]);
    s = add_if(s, 2 < k, G[3]);
    s = add_if(s, 3 < k, line[(t & 8u) ? 31 : 28]);
    s = add_if(s, 4 < k, line[29]);
    s = add_if(s, 5 < k, line[30]);
    uint32_t u = (1u << (levels - 6)) + (sl >> 6);
    for (int q = 6; q < k; q++) {
        s = add_if(s, true, heap[u]);
        u >>= 1;
    }
    return s;
}

int heap_emu_distances(const int32_t *parent, const float *distance, int64_t n_nodes, const int64_t *pairs, int64_t n,
                       double *out_d, int32_t *out_m)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return 1;
    if (!prepare_heap_lines(T)) { g_err = "heap lines not admitted"; return 2; }
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) { g_err = "id out of range"; return 3; }
        if ((a | b) & 1) {
            const PairResult r = pair_walk(T.nodes.data(), T.depth.data(), T.stride.data(), (int32_t)a, (int32_t)b);
            out_d[i] = (double)r.dist;
            out_m[i] = r.mrca;
            continue;
        }
        const uint32_t sa = (uint32_t)a >> 1, sb = (uint32_t)b >> 1, x = sa ^ sb;
        int k = 0;
        while (k < 32 && (x >> k)) k++;
        float s = 0.0f;
        s = side(T.heap_lines.data(), T.heap_dist.data(), T.heap_levels, sa, k, s);
        s = side(T.heap_lines.data(), T.heap_dist.data(), T.heap_levels, sb, k, s);
        out_d[i] = (double)s;
        out_m[i] = k ? (int32_t)((((((sa >> k) << 1) | 1u) << k)) - 1u) : (int32_t)a;
    }
    return 0;
}

}  // extern "C"
