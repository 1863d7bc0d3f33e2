// row_chunks.hpp — how the rows of one ingest / match call are cut into upload chunks, free of any device type (the library's
// RowUpload in bloomgpu.hip copies by this plan; tests/row_chunks_check.cpp runs the same code on the CPU, tests/test_row_chunks.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace bsh {

// Chunk c = rows [cuts[c], cuts[c + 1]).  `off` has n_rows + 1 ascending byte offsets (it need not start at 0).  The first chunk is
// small (the walk starts as soon as it has landed), every later one twice as large up to 4x: a launch must be big enough that each
// of the ~3 workgroups a CU holds walks several rows per lane, and the last chunk's walk is all that is left once the copy is over
// (2.5 GB of rows take ~50 ms over PCIe, their walk 12..30 ms — one after the other they would add up).
inline std::vector<uint32_t> plan_row_chunks(const uint64_t *off, uint32_t n_rows, uint64_t first_chunk_bytes)
{
    std::vector<uint32_t> cuts{0};
    uint64_t chunk_bytes = first_chunk_bytes;
    for (uint32_t r = 0; r < n_rows;) {
        const uint64_t lim = off[r] + chunk_bytes;
        if (chunk_bytes < 4 * first_chunk_bytes) chunk_bytes *= 2;
        uint32_t e = (uint32_t)(std::upper_bound(off + r + 1, off + n_rows + 1, lim) - off) - 1;
        e = std::max(e, r + 1);
        // whole 256-row workgroups per chunk (the last one takes what is left)
        if (e < n_rows) e = std::min<uint32_t>(n_rows, (e + 255u) / 256u * 256u);
        cuts.push_back(e);
        r = e;
    }
    return cuts;
}

// The bytes [b0, b1) chunk c brings, in the coordinates of `off`; n_bytes = off[n_rows], copied_to = the b1 of chunk c - 1 (chunks
// are copied in order).  The walker reads whole aligned 8-byte words, at most the word that holds a row's last byte: a chunk's
// range ends 16..23 bytes past its last row (rounded to 8) so that K(c) never touches a byte that has not landed — and the NEXT
// chunk starts exactly there, so no copy ever rewrites a byte a running kernel may be reading (the ranges are disjoint).
inline std::pair<uint64_t, uint64_t> chunk_copy_range(const uint64_t *off, const std::vector<uint32_t> &cuts, uint32_t c, uint64_t n_bytes,
                                                      uint64_t copied_to)
{
    const uint64_t b0 = c == 0 ? (off[cuts[c]] & ~7ull) : copied_to;
    return {b0, std::max(b0, std::min<uint64_t>(n_bytes, (off[cuts[c + 1]] + 23) & ~7ull))};
}

}  // namespace bsh
