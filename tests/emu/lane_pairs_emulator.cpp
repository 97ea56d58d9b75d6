// lane_pairs_emulator.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The shared line loads of k_canopy_ilp_heap's lane pairs on the host: a quad of four lanes over a table of heap lines, with
// the offset functions the kernel uses (suchtree_amd/csrc/tree_prep.h: heap_pair_offset and its helpers) and the exchange
// restated here -- lane l reads lane l ^ 1 for the neighbour's slot, issues the loads of step 0 and step 1, keeps the window,
// and hands the top it loaded back to the lane it belongs to.  The reference is what a lane read on its own before: the four
// floats at the window of its slot and the last four floats of its line.  Never loaded by suchtree_amd.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../suchtree_amd/csrc/tree_prep.h"

using namespace st;

extern "C" {

static std::string g_err;
const char *lane_pairs_last_error() { return g_err.c_str(); }

// heap_lines of a perfect tree (tree_prep.cpp: prepare_heap_lines) into out[n_out]; returns the floats written, or -1
int64_t lane_pairs_table(const int32_t *parent, const float *distance, int64_t n_nodes, float *out, int64_t n_out)
{
    TreeTables T;
    if (!prepare_basic(parent, distance, n_nodes, T, g_err)) return -1;
    if (!prepare_heap_lines(T) || (int64_t)T.heap_lines.size() > n_out) { g_err = "heap lines not admitted"; return -1; }
    std::memcpy(out, T.heap_lines.data(), T.heap_lines.size() * 4);
    return (int64_t)T.heap_lines.size();
}

// {window offset, top offset} of a slot, as the kernel computes them
void lane_pairs_offsets(uint32_t slot, uint32_t *out)
{
    out[0] = heap_window_offset(slot);
    out[1] = heap_top_offset(slot);
}

// which a lane of that parity reads in that step: 1 its own window, 0 its neighbour's top
int lane_pairs_reads_window(int step, int lane) { return heap_pair_window_mask(step, 0u - ((uint32_t)lane & 1u)) == 0xFFFFFFFFu ? 1 : 0; }

struct Lane {
    uint32_t slot, nb;
    float l[2][4];      // the loads of step 0 and 1
    float w[4], ntop[4], top[4];
};

// One quad with slots {q0, q1, q2, q3} on its lanes over `lines` (n_floats floats).  out[lane * 8 ..]: window then top as the
// lane holds them after the exchange; lines_touched[step]: distinct lines that step's loads of the quad touch.
// Returns 0, or 1 with an error when a load would leave the table.
int lane_pairs_quad(const float *lines, int64_t n_floats, const uint32_t *q, float *out, int32_t *lines_touched)
{
    Lane L[4];
    for (int l = 0; l < 4; l++) L[l].slot = q[l];
    for (int l = 0; l < 4; l++) L[l].nb = L[l ^ 1].slot;      // quad_perm:[1,0,3,2]
    for (int step = 0; step < 2; step++) {
        uint32_t seen[4];
        int n_seen = 0;
        for (int l = 0; l < 4; l++) {
            const uint32_t odd = 0u - ((uint32_t)l & 1u);
            const uint32_t off = heap_pair_offset(step, odd, L[l].slot, L[l].nb);
            if ((int64_t)off + 4 > n_floats) {
                g_err = "load past the table: offset " + std::to_string(off);
                return 1;
            }
            std::memcpy(L[l].l[step], lines + off, 16);
            bool dup = false;
            for (int k = 0; k < n_seen; k++) dup = dup || seen[k] == off / 32;
            if (!dup) seen[n_seen++] = off / 32;
        }
        lines_touched[step] = n_seen;
    }
    for (int l = 0; l < 4; l++) {
        const uint32_t odd = 0u - ((uint32_t)l & 1u);
        const uint32_t m = heap_pair_window_mask(1, odd);
        for (int c = 0; c < 4; c++) {
            uint32_t a, b, x, y;
            std::memcpy(&a, &L[l].l[0][c], 4);
            std::memcpy(&b, &L[l].l[1][c], 4);
            x = heap_pair_select(m, b, a);
            y = heap_pair_select(m, a, b);
            std::memcpy(&L[l].w[c], &x, 4);
            std::memcpy(&L[l].ntop[c], &y, 4);
        }
    }
    for (int l = 0; l < 4; l++) std::memcpy(L[l].top, L[l ^ 1].ntop, 16);
    for (int l = 0; l < 4; l++) {
        std::memcpy(out + 8 * l, L[l].w, 16);
        std::memcpy(out + 8 * l + 4, L[l].top, 16);
    }
    return 0;
}

// Every own slot x every neighbour slot of a table of n_slots leaf slots, the own slot on an even lane (0) and on an odd one
// (3) of the quad {own, nb, nb, own}: all four lanes must hold the eight floats a lane read on its own, and either step must
// touch two lines (one when both slots share a line).  Returns the number of quads that did not; the first one in the error.
int64_t lane_pairs_sweep(const float *lines, int64_t n_floats, uint32_t n_slots)
{
    int64_t bad = 0;
    for (uint32_t own = 0; own < n_slots; own++)
        for (uint32_t nb = 0; nb < n_slots; nb++) {
            const uint32_t q[4] = {own, nb, nb, own};
            float out[32];
            int32_t touched[2];
            if (lane_pairs_quad(lines, n_floats, q, out, touched)) return -1;
            bool ok = touched[0] == ((own >> 4) == (nb >> 4) ? 1 : 2) && touched[1] == touched[0];
            for (int l = 0; l < 4; l++) {
                const float *line = lines + (size_t)(q[l] >> 4) * 32;
                const uint32_t t = q[l] & 15u;
                const float *w = line + 7 * (t >> 2) + ((t & 2u) ? 3 : 0), *top = line + 28;      // (HeapSide::load before lane pairs)
                ok = ok && !std::memcmp(out + 8 * l, w, 16) && !std::memcmp(out + 8 * l + 4, top, 16);
            }
            if (!ok && !bad++) g_err = "own slot " + std::to_string(own) + ", neighbour slot " + std::to_string(nb);
        }
    return bad;
}

}  // extern "C"
