// build_plan.hpp — the arithmetic of the write side, free of any device type: how an arena's shard is laid out on one device and
// what the probe side is told about it, how a build call's descriptors are cut into per-device parts (word ranges, section
// regions, the words nobody owns), and by which route one filter is built.  bsg_arena_load, plan_arena, stream_finish, build_common
// and ingest_build_common (bloomgpu.hip, ingest_api.inc, stream_api.inc) plan by these functions; tests/build_plan_check.cpp runs
// the same code on the CPU (tests/test_build_plan.py).  Descriptors come in as the C-ABI's bsg_filter_desc; a shard's layout goes
// out as the same record (word_off, m, k) — the callers add the Barrett constant when they fill the device's DevDesc.
#pragma once
#include "bloomgpu.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bsh {

// bloomgpu.hip static_asserts these equal to its own
constexpr uint32_t kLdsBudget = 144 * 1024;            // dynamic LDS a workgroup may request
constexpr uint32_t kLdsCapWords = kLdsBudget / 8;      // largest bitset a probe stages in LDS
constexpr uint64_t kAlignWords = 16;                   // filters start on 128-byte boundaries in HBM
constexpr uint32_t kSetListBytes = 4 * 1024 * 4 + 16;  // static LDS of k_build_sets beside a staged bitset: its compaction list (ingest.hip.h)

inline uint64_t filter_words(uint64_t m) { return (m + 63) / 64; }
// words a filter takes in a 128-byte-aligned layout (a nil filter takes none)
inline uint64_t aligned_words(uint64_t m) { return m ? (filter_words(m) + kAlignWords - 1) / kAlignWords * kAlignWords : 0; }
inline uint64_t block_span_words(const bsg_filter_desc *d3) { return aligned_words(d3[0].m) + aligned_words(d3[1].m) + aligned_words(d3[2].m); }

// Section sizes are a function of the geometry alone: 1 + sum over present filters (4 + 24 + 8 * ceil(m/64)) + 4.
inline uint64_t section_len(const bsg_filter_desc *d3)
{
    uint64_t len = 1 + 4;
    for (int c = 0; c < 3; ++c)
        if (d3[c].m) len += 4 + 24 + 8 * filter_words(d3[c].m);
    return len;
}

// ---- an arena's shard on one device ----

// blocks of an arena of n_blocks that device di of nd holds: the global blocks di, di + nd, ...
inline uint32_t shard_blocks(uint32_t n_blocks, uint32_t di, uint32_t nd) { return n_blocks > di ? (n_blocks - di + nd - 1) / nd : 0; }

// What the probe side reads of a shard, per filter kind: probe launches size their LDS from max_staged_words, bsg_or_reduce
// refuses a kind whose geometry is not uniform.  fixed_m == 0 while uniform means "no filter seen yet": the first present filter
// is adopted, any later mismatch clears the flag for good.
struct ShardStats {
    uint64_t max_staged_words[3] = {0, 0, 0};
    uint64_t sum_words[3] = {0, 0, 0};  // present filters, for stream-byte accounting
    uint64_t fixed_m[3] = {0, 0, 0};    // common m if all present filters share geometry, else 0
    uint32_t fixed_k[3] = {0, 0, 0};
    bool geometry_uniform[3] = {true, true, true};
    uint32_t max_k[3] = {0, 0, 0};      // largest k of the present filters: the gather / stream decision of a probe launch (probe_plan.hpp)
    uint64_t sum_unstaged_words[3] = {0, 0, 0};   // the part of sum_words in filters beyond the LDS budget (never streamed: gathered per block)
    void add_filter(uint32_t c, uint64_t m, uint32_t k)
    {
        if (m == 0) return;
        const uint64_t nw = filter_words(m);
        sum_words[c] += nw;
        max_k[c] = std::max(max_k[c], k);
        if (nw <= kLdsCapWords) max_staged_words[c] = std::max(max_staged_words[c], nw);
        else sum_unstaged_words[c] += nw;
        if (fixed_m[c] == 0 && geometry_uniform[c]) { fixed_m[c] = m; fixed_k[c] = k; }
        else if (fixed_m[c] != m || fixed_k[c] != k) geometry_uniform[c] = false;
    }
};

struct ShardLayout {
    uint32_t n_blocks = 0;                    // local blocks: local lb is the global block lb * nd + di
    std::vector<bsg_filter_desc> filters;     // [n_blocks * 3] (word_off into the shard, m, k); a nil filter keeps word_off 0
    std::vector<uint64_t> block_off;          // [n_blocks] where a block's span of block_span_words() starts
    uint64_t n_words = 0;                     // the spans plus one alignment unit of padding behind the last
    ShardStats stats;
};

inline ShardLayout layout_shard(const bsg_filter_desc *desc, uint32_t n_blocks, uint32_t di, uint32_t nd)
{
    ShardLayout L;
    L.n_blocks = shard_blocks(n_blocks, di, nd);
    L.filters.resize((size_t)L.n_blocks * 3);
    L.block_off.resize(L.n_blocks);
    uint64_t cursor = 0;
    for (uint32_t lb = 0; lb < L.n_blocks; ++lb) {
        L.block_off[lb] = cursor;
        for (uint32_t c = 0; c < 3; ++c) {
            const bsg_filter_desc &f = desc[(size_t)(lb * nd + di) * 3 + c];
            L.filters[(size_t)lb * 3 + c] = bsg_filter_desc{f.m ? cursor : 0, f.m, f.k, 0};
            cursor += aligned_words(f.m);
            L.stats.add_filter(c, f.m, f.k);
        }
    }
    L.n_words = cursor + kAlignWords;
    return L;
}

// ---- the parts of a build call ----

// cuts [0, n) items with the given costs into at most `parts` contiguous runs of about equal cost; returns the run
// boundaries (size runs + 1).  `unit`: boundaries fall on multiples of it (3 = whole blocks of filters).
inline std::vector<uint32_t> balanced_cuts(const std::vector<uint64_t> &cost, uint32_t parts, uint32_t unit = 1)
{
    const uint32_t n = (uint32_t)cost.size();
    std::vector<uint32_t> cuts{0};
    uint64_t total = 0;
    for (uint64_t c : cost) total += c;
    uint64_t acc = 0;
    uint32_t made = 1;
    for (uint32_t i = 0; i < n && made < parts; ++i) {
        acc += cost[i];
        if ((i + 1) % unit == 0 && i + 1 < n && acc * parts >= total * made) { cuts.push_back(i + 1); ++made; }
    }
    cuts.push_back(n);
    return cuts;
}

// do the present filters' word offsets ascend with the index (each starts at or behind its predecessor's end)?  Only then do
// contiguous runs of descriptors own disjoint word ranges.
inline bool offsets_ascend(const bsg_filter_desc *desc, uint32_t n)
{
    uint64_t prev_end = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (desc[i].m == 0) continue;
        if (desc[i].word_off < prev_end) return false;
        prev_end = desc[i].word_off + filter_words(desc[i].m);
    }
    return true;
}

// One part: descriptors [i0, i1) of the call, built on one device.  Its filters occupy the words [w_lo, w_hi) of the caller's
// arena; with sections its blocks i0 / 3 .. i1 / 3 are serialised at region_off, region_len bytes.
struct PartSpan {
    uint32_t i0 = 0, i1 = 0;
    uint64_t w_lo = 0, w_hi = 0;
    uint64_t region_off = 0, region_len = 0;
};

// parts (PartSpan, or what the caller derives from it) come with i0 / i1 set and leave with their word range and section
// region; returns the bytes of all parts' sections (0 without sections).  Several parts own disjoint word ranges only where
// offsets_ascend() holds: a caller with more than one part asks that first.  A part without a present filter owns [0, 0); a
// single part owns the whole arena [0, n_words), which comes back zero-filled between the filters (the contract of the first,
// single-device build call).
template <class Part>
inline uint64_t plan_parts(const bsg_filter_desc *desc, std::vector<Part> &parts, uint64_t n_words, bool sections)
{
    uint64_t region_bytes = 0;
    for (PartSpan &P : parts) {
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t i = P.i0; i < P.i1; ++i) {
            if (desc[i].m == 0) continue;
            lo = std::min(lo, desc[i].word_off);
            hi = std::max(hi, desc[i].word_off + filter_words(desc[i].m));
        }
        if (lo == ~0ull) lo = hi = 0;
        if (parts.size() == 1) { lo = 0; hi = n_words; }
        P.w_lo = lo; P.w_hi = hi;
        P.region_off = P.region_len = 0;
        if (sections) {
            P.region_off = region_bytes;
            for (uint32_t b = P.i0 / 3; b < P.i1 / 3; ++b) P.region_len += section_len(desc + (size_t)b * 3);
            region_bytes += P.region_len;
        }
    }
    return region_bytes;
}

// do the parts' sections fit the region the caller gave?  (Here, not in the callers, so that the CPU test pins the edge.)
inline bool region_fits(uint64_t region_bytes, uint64_t region_cap) { return region_bytes <= region_cap; }

// words no part owns (gaps, absent filters) are zero, as the single-part call leaves them
template <class Part>
inline void zero_unowned(uint64_t *out_words, uint64_t n_words, const std::vector<Part> &parts)
{
    uint64_t at = 0;
    for (const PartSpan &P : parts) { if (P.w_lo > at) memset(out_words + at, 0, (P.w_lo - at) * 8); at = std::max(at, P.w_hi); }
    if (n_words > at) memset(out_words + at, 0, (n_words - at) * 8);
}

// a part's section offsets (relative to its region, one more than it has blocks) into the caller's list
inline void scatter_sec_off(uint64_t *sec_off, const PartSpan &P, const std::vector<uint64_t> &sec_off_local)
{
    for (uint32_t b = 0; b <= (P.i1 - P.i0) / 3; ++b) sec_off[P.i0 / 3 + b] = P.region_off + sec_off_local[b];
}

// ---- how one filter is built ----

enum class BuildRoute {
    Staged,      // the whole bitset is assembled in LDS by one workgroup
    Binned,      // beyond LDS: locations parked in HBM, the bitset assembled window by window (bin_build.hip.h)
    Sliced,      // beyond LDS, few locations: slices of the input set bits with global atomics
};

// lds_head_bytes: static LDS the build kernel keeps beside the staged bitset — 0 for k_build, k_build_sets' compaction list
// (kSetListBytes) on the tables route.  Binning pays from a few million locations on (three more launches, scratch from the
// pool); a bitset just beyond LDS with a few ten thousand entries stays L2-resident under its atomics.  bin_min_locs: fewest
// locations that are binned; bin_scratch_bytes: locations (4 bytes each) one binned build may park, 0 = never bin.
inline BuildRoute build_route(uint64_t m, uint64_t n_entries, uint64_t k, uint32_t lds_head_bytes, uint64_t bin_min_locs, uint64_t bin_scratch_bytes)
{
    if (filter_words(m) * 8 + lds_head_bytes <= kLdsBudget) return BuildRoute::Staged;
    const uint64_t n_locs = n_entries * k;
    const bool fits = m < (1ull << 31) && n_locs >= std::max<uint64_t>(bin_min_locs, 1) && n_locs < (1ull << 32) - 4096 &&
                      n_locs * 4 <= bin_scratch_bytes;
    return fits ? BuildRoute::Binned : BuildRoute::Sliced;
}

}  // namespace bsh
