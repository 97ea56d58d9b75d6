// heap_emulator.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Runs the product's heap-line tables (suchtree_amd/csrc/tree_prep.cpp: prepare_heap_lines) and the pair function of
// k_canopy_ilp_heap over them on the host (heap_pair_emu.h, with the six line values of a slot read straight out of its
// line).  Never loaded by suchtree_amd.
#include <cstdint>
#include <string>
#include <vector>

#include "heap_pair_emu.h"

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

int heap_emu_distances(const int32_t *parent, const float *distance, int64_t n_nodes, const int64_t *pairs, int64_t n,
                       double *out_d, int32_t *out_m)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return 1;
    if (!prepare_heap_lines(T)) { g_err = "heap lines not admitted"; return 2; }
    return heap_pairs_emu(T, n_nodes, pairs, n, out_d, out_m, g_err, [&T](uint32_t sl, float *e) {
        const float *line = T.heap_lines.data() + (size_t)(sl >> 4) * 32;
        const uint32_t t = sl & 15u;
        // (tree_prep.h: groups of four leaves at floats 7g .. 7g+6 -- own own h1 h2 h1 own own --, then e3 e4 e5 e3)
        const float *G = line + 7 * (t >> 2);
        const uint32_t r = t & 3u;
        e[0] = G[r < 2 ? r : r + 3];
        e[1] = G[r < 2 ? 2 : 4];
        e[2] = G[3];
        e[3] = line[(t & 8u) ? 31 : 28];
        e[4] = line[29];
        e[5] = line[30];
        return true;
    });
}

}  // extern "C"
