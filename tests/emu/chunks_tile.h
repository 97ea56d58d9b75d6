// What the sanitizer programs of the matrix plans share (sanitize_mantel.cpp, sanitize_group.cpp, sanitize_class.cpp,
// sanitize_parafit.cpp): the chunks of a plan tile every block of permutations once, in order.  block_tasks(n_perms) is
// the task count of a block of n_perms permutations; `chunk` is the call's chunk_tasks.  Prints the first condition that
// fails and returns 1; 0: every one holds.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../suchtree_amd/csrc/dispersion_plan.h"

#define TILE_CHECK(c)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <typename BlockTasks>
int chunks_tile(const st::MatrixPlan &P, int64_t chunk, BlockTasks block_tasks)
{
    int64_t p_next = 0, t_next = 0;
    for (const st::DispersionChunk &c : P.chunks) {
        TILE_CHECK(c.task_begin == t_next);
        if (t_next == 0) TILE_CHECK(c.p_begin == p_next);      // (a block begins where the one before ended)
        TILE_CHECK(c.n_perms >= 1 && c.n_perms <= P.perm_block && c.n_tasks >= 1 && c.n_tasks <= P.max_chunk_tasks);
        if (chunk > 0) TILE_CHECK(c.n_tasks <= chunk && c.n_perms <= chunk);
        t_next = c.task_begin + c.n_tasks;
        TILE_CHECK(t_next <= block_tasks(c.n_perms));
        if (t_next == block_tasks(c.n_perms)) {
            t_next = 0;
            p_next = c.p_begin + c.n_perms;
        }
    }
    TILE_CHECK(p_next == P.rows && t_next == 0);
    return 0;
}

#undef TILE_CHECK
