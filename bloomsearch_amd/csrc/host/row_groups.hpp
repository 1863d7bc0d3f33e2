// row_groups.hpp — the order in which a streaming ingest walks the rows of one upload chunk, free of any device type
// (bsg_ingest_append_rows in ingest_api.inc groups by this; tests/row_groups_check.cpp runs the same code on the CPU,
// tests/test_row_groups.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace bsh {

// First row whose set is not below n_sets, or n_rows when every row names an existing set (checked before anything is launched:
// the kernel indexes the table array with these values).
inline uint32_t first_bad_set(const uint32_t *set_of_row, uint32_t n_rows, uint32_t n_sets)
{
    for (uint32_t r = 0; r < n_rows; ++r)
        if (set_of_row[r] >= n_sets) return r;
    return n_rows;
}

// Rows [r0, r1) of a batch, stably grouped by set: order[r0 .. r1) receives a permutation of r0 .. r1 - 1 in which the sets
// ascend and the rows of one set keep their arrival order, set_of_order[i] = set_of_row[order[i]].  Nothing outside [r0, r1) of
// either output is touched and no row byte moves.  Every set_of_row[r] must be < n_sets (first_bad_set).
// A counting sort over the sets that exist; when they far outnumber the chunk's rows (a small batch of an ingest with very many
// partitions) a stable sort of the indices instead, so that the cost follows the rows and not the sets.  `counts` is scratch the
// caller keeps between chunks.
inline void group_rows_by_set(const uint32_t *set_of_row, uint32_t r0, uint32_t r1, uint32_t n_sets, uint32_t *order, uint32_t *set_of_order,
                              std::vector<uint32_t> &counts)
{
    const uint32_t n = r1 - r0;
    if (n == 0) return;
    if ((uint64_t)n_sets > (uint64_t)n * 4) {
        std::iota(order + r0, order + r1, r0);
        std::stable_sort(order + r0, order + r1, [&](uint32_t x, uint32_t y) { return set_of_row[x] < set_of_row[y]; });
    } else {
        counts.assign((size_t)n_sets + 1, 0);
        for (uint32_t r = r0; r < r1; ++r) counts[set_of_row[r] + 1] += 1;
        for (uint32_t s = 0; s < n_sets; ++s) counts[s + 1] += counts[s];      // counts[s] = first position of set s within the chunk
        for (uint32_t r = r0; r < r1; ++r) order[r0 + counts[set_of_row[r]]++] = r;
    }
    for (uint32_t i = r0; i < r1; ++i) set_of_order[i] = set_of_row[order[i]];
}

}  // namespace bsh
