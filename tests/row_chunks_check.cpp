// Host driver of the row-upload chunk plan (bloomsearch_amd/csrc/host/row_chunks.hpp — the code the library's RowUpload copies by),
// built with plain g++ by tests/test_row_chunks.py.  Input file: little-endian u64 words — the number of cases, then per case
// first_chunk_bytes, n_rows and n_rows + 1 offsets.  Output per case: one line of cuts, one line of "b0 b1" pairs per chunk.
#include "host/row_chunks.hpp"
#include <cstdio>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n_cases = 0;
    if (fread(&n_cases, 8, 1, f) != 1) return 2;
    for (uint64_t i = 0; i < n_cases; ++i) {
        uint64_t head[2];
        if (fread(head, 8, 2, f) != 2) return 2;
        const uint32_t n_rows = (uint32_t)head[1];
        std::vector<uint64_t> off((size_t)n_rows + 1);
        if (fread(off.data(), 8, off.size(), f) != off.size()) return 2;
        const std::vector<uint32_t> cuts = bsh::plan_row_chunks(off.data(), n_rows, head[0]);
        for (uint32_t c : cuts) printf("%u ", c);
        printf("\n");
        uint64_t copied_to = 0;
        for (uint32_t c = 0; c + 1 < cuts.size(); ++c) {
            const auto [b0, b1] = bsh::chunk_copy_range(off.data(), cuts, c, off[n_rows], copied_to);
            copied_to = b1;
            printf("%llu %llu ", (unsigned long long)b0, (unsigned long long)b1);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
