// rf_plan.h -- the host-only side of the batched exact clade comparison of a set of trees (st_rf_tasks: compare.tree_set,
// compare.rf_relabelled), plain C++17, and what the device shares with it (kernels_rf.h): the limits, the LDS layout, the
// key of a range, the extrema of a range of positions and the test of one clade.  No GPU calls in here (rf_plan.cpp): the
// "not gpu" tests run it under the address / undefined-behaviour sanitizers (tests/emu/sanitize_rf.cpp).  The definitions
// are the contract of include/suchtree_hip.h (st_rf_tasks).
//
// Day's method.  A task is (tree i, tree j, alignment a).  q[y] is the position in i of the leaf at position y of j: one
// scatter of m 16-bit entries.  Clade b = [lo, hi) of j is the set Q_b = q[lo .. hi) of i's positions, and Q_b is a clade
// of i if and only if it is contiguous -- max - min + 1 = size, q being a permutation -- and the range [min, max + 1) is
// in i's list.  The extrema of a range are two partial blocks of 64 positions and two entries of a sparse table over the
// whole blocks between them (level l, block b: the extrema of blocks [b, b + 2^l)).  i's list is looked up by binary
// search in its keys, sorted once per call.  Unrooted, a set and its complement are one bipartition: every key is that
// of the side without i's position 0, so a clade of j that holds the leaf at i's position 0 (the noted leaf) is tested
// through its complement [0, lo) + [hi, m), and a range of i's list that starts at 0 is stored as [hi, m).
// Everything is an integer: tasks, chunks and the grid give the same counts.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "plan_checks.h"

namespace st {

constexpr int32_t kRfMinLeaves = 4;
constexpr int32_t kRfMaxLeaves = ST_RF_MAX_LEAVES;
constexpr int kRfThreads = 256;                  // the workgroup of k_rf_tasks: four waves
constexpr int kRfBlocks = 4096;                  // the grid's cap: a workgroup strides over a chunk's tasks
constexpr int64_t kRfChunkTasks = 65536;         // default tasks per chunk
constexpr int64_t kRfChunkTasksMax = 1 << 24;    // a larger chunk_tasks is cut to this: a launch counts its tasks in an int32
constexpr uint32_t kRfNoKey = ~(uint32_t)0;      // the key of a set that is no range

// blocks of 64 positions (at most 256), the table's row stride in entries (rows start on 16 bytes) and its levels (at most 9)
ST_QUARTET_HD int rf_blocks(int m) { return (m + 63) >> 6; }
ST_QUARTET_HD int rf_stride(int nb) { return (nb + 7) & ~7; }
ST_QUARTET_HD int rf_levels(int nb)
{
    int l = 1;
    while ((1 << l) <= nb) l++;
    return l;
}

// LDS of a workgroup, all of it dynamic: 16 bytes where the waves meet (the task's count, the noted position), the minima
// and the maxima of the table (levels x stride uint16 each), then q, m uint16 rounded up to 16 bytes.  At the cap:
// 16 + 2 * 9 * 256 * 2 + 32768 = 42,000 bytes.
ST_QUARTET_HD size_t rf_lds_table(int m) { return (size_t)rf_levels(rf_blocks(m)) * (size_t)rf_stride(rf_blocks(m)) * 2; }
ST_QUARTET_HD size_t rf_lds_bytes(int m) { return 16 + 2 * rf_lds_table(m) + (((size_t)m + 7) & ~(size_t)7) * 2; }

// hi <= 16384 = 2^14: both ends fit 16 bits
ST_QUARTET_HD uint32_t rf_key(int lo, int hi) { return ((uint32_t)lo << 16) | (uint32_t)hi; }

// the key under which a range of tree i's list is stored: itself, or unrooted the side without position 0
ST_QUARTET_HD uint32_t rf_canonical(int lo, int hi, int m, bool unrooted) { return unrooted && lo == 0 ? rf_key(hi, m) : rf_key(lo, hi); }

// mn / mx joined with the extrema of q[lo .. hi), 0 <= lo < hi <= m.  A scan of a partial block stops once mx - mn >= limit:
// the caller's set is then no range of `limit` positions, whatever follows.  At most 126 entries are read one by one.
ST_QUARTET_HD void rf_extrema(const uint16_t *q, const uint16_t *tmin, const uint16_t *tmax, int stride, int lo, int hi, int limit, int &mn, int &mx)
{
    const int bl = (lo + 63) >> 6, bh = hi >> 6;      // whole blocks [bl, bh)
    if (bl < bh) {
        const int l = 31 - __builtin_clz((unsigned)(bh - bl)), x = l * stride + bl, y = l * stride + bh - (1 << l);
        const int a = tmin[x] < tmin[y] ? tmin[x] : tmin[y], b = tmax[x] > tmax[y] ? tmax[x] : tmax[y];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int head_end = bl * 64 < hi ? bl * 64 : hi, tail = bh * 64 > head_end ? bh * 64 : head_end;
    for (int k = lo; k < head_end && mx - mn < limit; k++) {
        const int v = q[k];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int k = tail; k < hi && mx - mn < limit; k++) {
        const int v = q[k];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
}

// The key of Q_b for clade [lo, hi) of tree j, or kRfNoKey when the set is no range of tree i's positions.  Unrooted, with
// the noted position inside, the complement is taken; the complement of everything is the empty range [m, m).
ST_QUARTET_HD uint32_t rf_clade_key(const uint16_t *q, const uint16_t *tmin, const uint16_t *tmax, int stride, int m, int lo, int hi, bool unrooted, int noted)
{
    int mn = m, mx = -1, s = hi - lo;
    if (unrooted && lo <= noted && noted < hi) {
        s = m - s;
        if (s == 0) return rf_key(m, m);
        if (lo > 0) rf_extrema(q, tmin, tmax, stride, 0, lo, s, mn, mx);
        if (hi < m && mx - mn < s) rf_extrema(q, tmin, tmax, stride, hi, m, s, mn, mx);
    } else {
        rf_extrema(q, tmin, tmax, stride, lo, hi, s, mn, mx);
    }
    return mx - mn + 1 == s ? rf_key(mn, mx + 1) : kRfNoKey;
}

// the first entry of the sorted keys[0 .. n) that equals `key`, or -1: at most 32 halvings
ST_QUARTET_HD int rf_find(const uint32_t *keys, int n, uint32_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && keys[lo] == key ? lo : -1;
}

// What a call uploads: the positions and the alignments as 16-bit entries, per clade of the concatenated list its range
// (lo << 16 | hi, as given), and per tree its canonical keys in increasing order with the index in the tree's list beside
// each (equal keys keep the list's order, so the first of them is the first of the list).
struct RfPlan {
    int32_t m = 0, n_trees = 0, n_align = 0;
    bool unrooted = false, triangle = false;
    int64_t n_tasks = 0, begin = 0, chunk = 0;      // chunk: tasks per launch, >= 1
    int64_t n_clades = 0;
    std::vector<uint16_t> where, align;
    std::vector<int32_t> off;                        // n_trees + 1
    std::vector<uint32_t> range, key;
    std::vector<int32_t> idx;
};

// ST_OK with the plan, or ST_ERR_ARG / ST_ERR_BOUNDS with `err`.  Checks, in this order: m in range; no negative count,
// begin or chunk; NULL arrays; the offsets (from 0, non-decreasing, below 2^31); every row of `where` a permutation of
// 0 .. m - 1; every range 0 <= lo < hi <= m; every row of `align` a permutation; then the tasks -- explicit: task_i and
// task_j given together, begin = 0, every tree index and alignment index in range (ST_ERR_BOUNDS, naming the task);
// triangle: [begin, begin + n_tasks) inside n_trees (n_trees - 1) / 2 -- and out_shared.
int rf_plan(int32_t m, int32_t n_trees, const int32_t *where, const int64_t *clade_offsets, const int32_t *lo, const int32_t *hi, bool unrooted,
            const int32_t *align, int32_t n_align, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int64_t n_tasks,
            int64_t begin, int64_t chunk_tasks, const int32_t *out_shared, RfPlan &P, std::string &err);

// task t of the call: (i, j, p), p = -1 for the identity
inline void rf_task(const RfPlan &P, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int64_t t, int32_t &i, int32_t &j, int32_t &p)
{
    if (P.triangle) {
        int64_t a, b;
        unifrac_pair(P.begin + t, a, b);
        i = (int32_t)a;
        j = (int32_t)b;
        p = -1;
    } else {
        i = task_i[t];
        j = task_j[t];
        p = task_p ? task_p[t] : -1;
    }
}

// the kernel's method on the host, one thread: out_shared[t] per task, out_count (may be NULL) zeroed and then added to
void rf_host(const RfPlan &P, const int32_t *task_i, const int32_t *task_j, const int32_t *task_p, int32_t *out_shared, int64_t *out_count);

}  // namespace st
