// host_options.h -- part of suchtree_hip.hip (included behind host_tree.h).
// The handle options of st_tree_set_option: one row per option -- its name, the member of st_tree it sets and its rule -- and
// the one function that looks a name up, checks the rule and stores.  A new option is a member in st_tree.h and a row here.
#pragma once

// value must lie in [lo, hi]; `must` is how the message says so ("<name> must be <must>")
struct OptionRule {
    int64_t lo, hi;
    const char *must;
};
static const OptionRule kOptZeroOne{0, 1, "0 or 1"};
static const OptionRule kOptZeroToTwo{0, 2, "0, 1 or 2"};
static const OptionRule kOptSortTile{0, 4, "0, 1, 2 or 4"};      // (and not 3)
static const OptionRule kOptNotNegative{0, std::numeric_limits<int64_t>::max(), ">= 0"};
static const OptionRule kOptMeasure{0, 7, "a combination of 1 (trace), 2 (skip CPU passes), 4 (skip GPU side)"};      // (host_path.h::run_pipe)
static const OptionRule kOptReserveCus{0, 0, "in [0, CUs of the device)"};      // (hi: the handle's n_cu_device - 1)
static const OptionRule kOptAny{std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max(), ""};

struct OptionRow {
    const char *name;
    int st_tree::*i32;          // the member the option sets: this one ...
    int64_t st_tree::*i64;      // ... or this one
    const OptionRule *rule;
};
#define ST_OPTION(member, rule) {#member, &st_tree::member, nullptr, &rule}
#define ST_OPTION64(member, rule) {#member, nullptr, &st_tree::member, &rule}
static const OptionRow kOptions[] = {
    ST_OPTION(tile_sort, kOptZeroOne),
    ST_OPTION(ladder_scalar, kOptZeroOne),
    // the persistent kernels are sized to the CUs of the device; on a rank that also receives (the root of the
    // multi-GPU gather) RCCL's kernels need somewhere to run beside a 1024-lane / 144 KiB workgroup per CU
    {"reserve_cus", &st_tree::n_cu, nullptr, &kOptReserveCus},      // (stores n_cu_device - value)
    ST_OPTION(ladder_dynamic, kOptZeroOne),
    ST_OPTION(cherries, kOptZeroOne),
    ST_OPTION(heap_lines, kOptZeroToTwo),
    ST_OPTION(heap_codes, kOptZeroToTwo),
    ST_OPTION(stream_hint, kOptZeroToTwo),
    ST_OPTION(batch_probe, kOptZeroOne),
    ST_OPTION(measure, kOptMeasure),
    ST_OPTION64(ladder_min_pairs, kOptNotNegative),
    ST_OPTION(tree_rmq, kOptZeroOne),
    ST_OPTION(mrca_ranks, kOptZeroOne),
    ST_OPTION(rec_a4, kOptZeroOne),
    ST_OPTION(walk_ladder, kOptZeroOne),
    ST_OPTION(prefer_walk_sorted, kOptZeroOne),
    ST_OPTION(wire48, kOptZeroOne),
    ST_OPTION(wire24, kOptZeroOne),
    ST_OPTION(sort_tile, kOptSortTile),
    ST_OPTION64(walk_sort_min, kOptNotNegative),
    ST_OPTION(walk_crown, kOptZeroOne),
    ST_OPTION(walk_sort, kOptZeroOne),
    ST_OPTION(lineage_lens, kOptZeroOne),
    ST_OPTION(lineage_sums, kOptZeroOne),
    ST_OPTION(ladder_sums, kOptZeroOne),      // (also clears ladder_sums_max_pairs)
    ST_OPTION(small_batch_path, kOptAny),     // (stores value != 0)
};
#undef ST_OPTION
#undef ST_OPTION64

// One option of one replica; st_tree_set_option applies it to every replica of the handle.
static int set_option_one(st_tree *t, const char *name, int64_t value)
{
    const OptionRow *row = nullptr;
    for (const OptionRow &r : kOptions)
        if (std::strcmp(name, r.name) == 0) row = &r;
    if (!row) return fail(ST_ERR_ARG, std::string("unknown option ") + name);
    const OptionRule &rule = *row->rule;
    const int64_t hi = &rule == &kOptReserveCus ? (int64_t)t->n_cu_device - 1 : rule.hi;
    if (value < rule.lo || value > hi || (&rule == &kOptSortTile && value == 3))
        return fail(ST_ERR_ARG, std::string(name) + " must be " + rule.must);
    if (row->i64) t->*row->i64 = value;
    else t->*row->i32 = (int)value;
    // the three that store something beside, or other than, their value
    if (&rule == &kOptReserveCus) t->n_cu = t->n_cu_device - (int)value;
    if (&rule == &kOptAny) t->small_batch_path = value != 0;
    if (row->i32 == &st_tree::ladder_sums) t->ladder_sums_max_pairs = 0;      // (an explicit setting holds for every batch size)
    return ST_OK;
}
