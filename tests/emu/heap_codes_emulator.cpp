// heap_codes_emulator.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Runs the product's heap-code table (suchtree_amd/csrc/tree_prep.cpp: prepare_heap_codes) and the place, extraction and
// decoding functions k_canopy_ilp_codes uses over it (tree_prep.h) on the host: a lane's two loads become bounds-checked
// copies of 16 bytes out of the table (on the lane itself, and shared between two lanes as CodeSide shares them), everything after them is the kernel's own code.  codes_emu_distances is the
// kernel's pair function over the table and the heap image (heap_pair_emu.h).  Never loaded by suchtree_amd.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "heap_pair_emu.h"

using namespace st;

static std::string g_err;

// One 16-byte load of the kernel at dword `word`; false when it would leave the allocation or its 128-byte line.
static bool load16(const uint32_t *table, int64_t n_words, uint32_t word, uint32_t d[4])
{
    if ((int64_t)word + 4 > n_words) { g_err = "a load at dword " + std::to_string(word) + " reaches past the table"; return false; }
    if ((word >> 5) != ((word + 3) >> 5)) { g_err = "a load at dword " + std::to_string(word) + " leaves its line"; return false; }
    std::memcpy(d, table + word, 16);
    return true;
}

// The six codes of a slot's lineage with both loads on the slot's own lane; false when a load would leave the allocation.
static bool slot_codes(const uint32_t *table, int64_t n_words, uint32_t slot, uint32_t c[6])
{
    const HeapCodePlace w = heap_code_window_place(slot), t = heap_code_top_place(slot);
    uint32_t d[4], e[4];
    if (!load16(table, n_words, w.word, d) || !load16(table, n_words, t.word, e)) return false;
    if (w.phase >= 32u || (t.phase != 12u && t.phase != 24u && t.phase != 64u)) { g_err = "phase out of range at slot " + std::to_string(slot); return false; }
    const HeapCodeTriple lo = heap_code_window_fields(d[0], d[1], d[2], d[3], w.phase, slot);
    const HeapCodeTopBits n = heap_code_top_bits(e[0], e[1], e[2], e[3], t.phase);
    const HeapCodeTriple hi = heap_code_top_fields(n.n0, n.n1);
    c[0] = lo.c0; c[1] = lo.c1; c[2] = lo.c2;
    c[3] = hi.c0; c[4] = hi.c1; c[5] = hi.c2;
    return true;
}

// The same for the two slots of lanes l (even) and l ^ 1 (odd) the way CodeSide does it (kernels_canopy_codes.h): step 0 and 1
// each read one slot's window on its own lane and its top on the other lane, the loading lane shifts the top down and hands
// two dwords over.  lines[step] = distinct 128-byte lines the two lanes touched in that step.
static bool lane_pair_codes(const uint32_t *table, int64_t n_words, const uint32_t slot[2], uint32_t c[2][6], int lines[2])
{
    uint32_t ld[2][2][4];      // [lane][step]
    for (int lane = 0; lane < 2; lane++) {
        const uint32_t odd = lane ? 0xFFFFFFFFu : 0u;
        for (int step = 0; step < 2; step++)
            if (!load16(table, n_words, heap_code_pair_word(step, odd, slot[lane], slot[lane ^ 1]), ld[lane][step])) return false;
    }
    for (int step = 0; step < 2; step++) {
        const uint32_t w0 = heap_code_pair_word(step, 0u, slot[0], slot[1]), w1 = heap_code_pair_word(step, 0xFFFFFFFFu, slot[1], slot[0]);
        lines[step] = (w0 >> 5) == (w1 >> 5) ? 1 : 2;
    }
    uint32_t win[2][4], bits[2][2];      // each lane's own window; the NEIGHBOUR's top bits as the lane computed them
    for (int lane = 0; lane < 2; lane++) {
        const uint32_t odd = lane ? 0xFFFFFFFFu : 0u, m = heap_pair_window_mask(1, odd);
        uint32_t t[4];
        for (int j = 0; j < 4; j++) {
            t[j] = heap_pair_select(m, ld[lane][0][j], ld[lane][1][j]);
            win[lane][j] = heap_pair_select(m, ld[lane][1][j], ld[lane][0][j]);
        }
        const HeapCodeTopBits n = heap_code_top_bits(t[0], t[1], t[2], t[3], heap_code_top_place(slot[lane ^ 1]).phase);
        bits[lane][0] = n.n0;
        bits[lane][1] = n.n1;
    }
    for (int lane = 0; lane < 2; lane++) {      // (the swap: a lane takes what the other one computed)
        const HeapCodeTriple lo = heap_code_window_fields(win[lane][0], win[lane][1], win[lane][2], win[lane][3],
                                                          heap_code_window_place(slot[lane]).phase, slot[lane]);
        const HeapCodeTriple hi = heap_code_top_fields(bits[lane ^ 1][0], bits[lane ^ 1][1]);
        c[lane][0] = lo.c0; c[lane][1] = lo.c1; c[lane][2] = lo.c2;
        c[lane][3] = hi.c0; c[lane][4] = hi.c1; c[lane][5] = hi.c2;
    }
    return true;
}

extern "C" {

const char *codes_emu_last_error() { return g_err.c_str(); }

// out[i] = the length code c[i] stands for: f32 = 0 by the definition, 1 by the float32 sequence of the kernel
void codes_emu_decode(const uint32_t *c, int64_t n, int f32, float *out)
{
    for (int64_t i = 0; i < n; i++) out[i] = f32 ? heap_code_decode_f32(c[i]) : heap_code_decode(c[i]);
}

// 1 and *c = its code if x has one, else 0
int codes_emu_code_of(float x, uint32_t *c) { return heap_code_of(x, *c) ? 1 : 0; }

// Returns 0 both tables built, 1 bad tree, 2 no heap lines, 3 heap lines without codes.
// sizes = {floats of heap_lines, words of heap_codes, levels}.  words: the table, if it fits cap.
int codes_emu_prepare(const int32_t *parent, const float *distance, int64_t n_nodes, int64_t *sizes, uint32_t *words, int64_t cap)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return 1;
    const bool lines = prepare_heap_lines(T);
    const bool codes = lines && prepare_heap_codes(T);
    sizes[0] = (int64_t)T.heap_lines.size();
    sizes[1] = (int64_t)T.heap_codes.size();
    sizes[2] = T.heap_levels;
    if (codes && words && (int64_t)T.heap_codes.size() <= cap) std::memcpy(words, T.heap_codes.data(), T.heap_codes.size() * 4);
    return !lines ? 2 : codes ? 0 : 3;
}

// The six lowest edges of a leaf slot's lineage as the kernel finds them in `table` (n_words words): 0, or 1 when a load
// would leave the allocation or its line.
int codes_emu_lineage(const uint32_t *table, int64_t n_words, uint32_t slot, float *out6)
{
    uint32_t c[6];
    if (!slot_codes(table, n_words, slot, c)) return 1;
    for (int j = 0; j < 6; j++) out6[j] = heap_code_decode_f32(c[j]);
    return 0;
}

// Every (even lane's slot, odd lane's slot) of n_slots x n_slots through the lane-pair form against the one-lane form: returns
// the number of lane pairs that differ or touch more than one line per step and lane ... 0, or -1 on a refused load.
int64_t codes_emu_lane_pairs(const uint32_t *table, int64_t n_words, uint32_t n_slots)
{
    int64_t bad = 0;
    for (uint32_t s0 = 0; s0 < n_slots; s0++)
        for (uint32_t s1 = 0; s1 < n_slots; s1++) {
            const uint32_t slot[2] = {s0, s1};
            uint32_t c[2][6], want[2][6];
            int lines[2];
            if (!lane_pair_codes(table, n_words, slot, c, lines) || !slot_codes(table, n_words, s0, want[0]) || !slot_codes(table, n_words, s1, want[1])) return -1;
            // step 0 serves the even lane's slot, step 1 the odd lane's: both lanes of a step are on ONE line
            if (std::memcmp(c, want, sizeof c) != 0 || lines[0] != 1 || lines[1] != 1) bad++;
        }
    return bad;
}

int codes_emu_distances(const int32_t *parent, const float *distance, int64_t n_nodes, const int64_t *pairs, int64_t n,
                        double *out_d, int32_t *out_m)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return 1;
    if (!prepare_heap_lines(T) || !prepare_heap_codes(T)) { g_err = "heap codes not admitted"; return 2; }
    return heap_pairs_emu(T, n_nodes, pairs, n, out_d, out_m, g_err, [&T](uint32_t sl, float *e) {
        uint32_t c[6];
        if (!slot_codes(T.heap_codes.data(), (int64_t)T.heap_codes.size(), sl, c)) return false;
        for (int j = 0; j < 6; j++) e[j] = heap_code_decode_f32(c[j]);
        return true;
    });
}

}  // extern "C"
