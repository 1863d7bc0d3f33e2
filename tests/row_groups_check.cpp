// Host driver of the walking order of a streaming ingest's upload chunks (bloomsearch_amd/csrc/host/row_groups.hpp — the code
// bsg_ingest_append_rows groups every chunk by), built with plain g++ under -fsanitize=address,undefined by tests/test_row_groups.py.
// Input file: little-endian u32 words — the number of cases, then per case n_sets, n_rows, r0, r1 and n_rows set indices.
// Output per case: first_bad_set; unless a set is out of range, the order of [r0, r1), its sets, and 1 when nothing outside
// [r0, r1) of either output was written.
#include "host/row_groups.hpp"
#include <cstdio>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    std::vector<uint32_t> counts;                              // kept between cases, as the library keeps it between chunks
    for (uint32_t i = 0; i < n_cases; ++i) {
        uint32_t head[4];
        if (fread(head, 4, 4, f) != 4) return 2;
        const uint32_t n_sets = head[0], n_rows = head[1], r0 = head[2], r1 = head[3];
        std::vector<uint32_t> set_of_row(n_rows);
        if (n_rows && fread(set_of_row.data(), 4, n_rows, f) != n_rows) return 2;
        const uint32_t bad = bsh::first_bad_set(set_of_row.data(), n_rows, n_sets);
        printf("%u\n", bad);
        if (bad < n_rows) continue;
        std::vector<uint32_t> order(n_rows, 0xFFFFFFFFu), sets(n_rows, 0xFFFFFFFFu);
        bsh::group_rows_by_set(set_of_row.data(), r0, r1, n_sets, order.data(), sets.data(), counts);
        for (uint32_t r = r0; r < r1; ++r) printf("%u ", order[r]);
        printf("\n");
        for (uint32_t r = r0; r < r1; ++r) printf("%u ", sets[r]);
        printf("\n");
        bool untouched = true;
        for (uint32_t r = 0; r < n_rows; ++r)
            if ((r < r0 || r >= r1) && (order[r] != 0xFFFFFFFFu || sets[r] != 0xFFFFFFFFu)) untouched = false;
        printf("%d\n", untouched ? 1 : 0);
    }
    fclose(f);
    return 0;
}
