// probe_plan.hpp — the arithmetic of a probe call, free of any device type: where the survivors of every arena go, how one device's
// shards are cut into launch groups, the tail-split cut, the layout of survivor rows, and the host merge of the per-device bitsets.
// probe_arenas / query_solo (probe_api.inc) plan and merge by these functions; tests/probe_plan_check.cpp runs the same code on the
// CPU (tests/test_probe_plan.py).  Everything here works on block counts and sizes only; a list of block counts is taken as a
// callable i -> blocks (the library reads them out of its arenas in place, the test out of a vector).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsh {

// bytes of survivors / verdict words one dispatch group may need (a single arena beyond it still forms a group)
constexpr uint64_t kGroupScratchBudget = 256ull << 20;

inline uint32_t words64(uint64_t n_blocks) { return (uint32_t)((n_blocks + 63) / 64); }

// [n_arenas + 1] word offsets: arena i's survivors ([n_queries][ceil(blocks / 64)]) start at out + offsets[i]
template <class BlocksOf>
inline std::vector<uint64_t> survivor_offsets(uint32_t n_arenas, uint32_t n_queries, BlocksOf &&blocks)
{
    std::vector<uint64_t> off(n_arenas + 1, 0);
    for (uint32_t i = 0; i < n_arenas; ++i) off[i + 1] = off[i] + (uint64_t)n_queries * words64(blocks(i));
    return off;
}

// A launch group as numbers: the shards (on one device) of some arenas of the caller's list, probed by ONE dispatch.
struct GroupPlan {
    std::vector<uint32_t> index;     // position of each shard's arena in the caller's list
    uint64_t v_words = 0;            // verdict scratch the group needs (u64)
    uint64_t out_words = 0;          // survivors the group produces (u64)
    uint32_t max_blocks = 0, max_G = 0, total_G = 0;
    void add(uint32_t pos, uint32_t n_blocks, uint32_t n_queries, uint32_t Wt)
    {
        const uint32_t G = words64(n_blocks);
        index.push_back(pos);
        v_words += (uint64_t)G * std::max(Wt, 1u) * 64;
        out_words += (uint64_t)n_queries * G;
        max_blocks = std::max(max_blocks, n_blocks);
        max_G = std::max(max_G, G);
        total_G += G;
    }
};

// The groups of one device from its local block counts per arena (empty shards join no group).  A group closes when it holds
// `limit` shards, and also on BYTES: its survivors (n_queries x 64-block groups x 8) and verdict words live in scratch that never
// shrinks, and one huge group is one copy behind one dispatch — nothing for the copy stream to overlap.  A single shard beyond the
// budget still forms a group.  G: GroupPlan, or what the caller derives from it.
template <class G = GroupPlan, class BlocksOf>
inline std::vector<G> plan_groups(uint32_t n_arenas, BlocksOf &&local_blocks, uint32_t n_queries, uint32_t Wt, uint32_t limit,
                                  uint64_t budget = kGroupScratchBudget)
{
    std::vector<G> groups;
    for (uint32_t i = 0; i < n_arenas; ++i) {
        const uint32_t n_blocks = local_blocks(i);
        if (n_blocks == 0) continue;
        const uint64_t G_add = words64(n_blocks);
        const bool full = !groups.empty() && !groups.back().index.empty() &&
                          ((groups.back().out_words + (uint64_t)n_queries * G_add) * 8 > budget ||
                           (groups.back().v_words + G_add * std::max(Wt, 1u) * 64) * 8 > budget);
        if (groups.empty() || groups.back().index.size() >= limit || full) groups.emplace_back();
        groups.back().add(i, n_blocks, n_queries, Wt);
    }
    return groups;
}

// [n_groups + 1] where each group's survivors go (u64 offset).  out_off != nullptr (one device, or survivors left on the device):
// a group's arenas are consecutive in the caller's list unless empty arenas sit between them (those produce no words), so the
// group's words are contiguous at out_off[first arena of the group]; the last entry stays 0.  out_off == nullptr (several devices,
// host output): a running sum inside the device's own part buffer, the last entry its size.
template <class G>
inline std::vector<uint64_t> group_offsets(const std::vector<G> &groups, const uint64_t *out_off)
{
    std::vector<uint64_t> goff(groups.size() + 1, 0);
    uint64_t total = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        goff[gi] = out_off ? out_off[groups[gi].index[0]] : total;
        total += groups[gi].out_words;
    }
    if (!out_off) goff[groups.size()] = total;
    return goff;
}

// Gather or stream (the few-term probe of a launch group).  A filter kind of the group is cheaper to GATHER — terms x k word loads per
// block, each costing `gather_cost` bytes of memory traffic — than to stream when
//     terms x k x gather_cost x n_blocks  <  sum_words x 8          (strictly: equality streams)
// with sum_words the u64 words of that kind's filters over the group's blocks and k the largest k among them.  The whole launch takes
// the gather kernel only when EVERY referenced kind satisfies it and the batch is a few-term batch (the many-term kernels compact
// their survivors in LDS: there is no gathered form of them).  A kind whose filters are all nil (sum_words 0) never satisfies it, nor
// does a group without blocks; cost 0 gathers whatever has bytes.
// Filters beyond the LDS budget (unstaged_words) are never streamed: k_probe_terms gathers them per block already, the rule's bytes
// are not what the launch would otherwise move, and measured (profiles/probe_gather_lab.txt, big_filters geometry) the gather kernel
// is a draw up to 29 terms and 1-3 us behind from 48 — a launch that holds one keeps the streaming kernels unless the cost is 0.
// (unstaged_words counts by the library's fixed staging cap, bsh::kLdsCapWords.  A launch's own cap is a little lower — the LDS
// budget minus its verdict words and wave queues — so a filter between the two is gathered per block by k_probe_terms and still
// counts as staged here: the byte rule then decides for it as for any other filter.)
// The left side is formed in 128 bits and saturates: terms, k and cost are 32-bit and n_blocks is 64-bit, so the plain product can
// pass 2^64 (and, for arguments no launch has, 2^128).
struct GatherKind {
    uint64_t sum_words;        // u64 words of this kind's filters over every block of the group
    uint64_t unstaged_words;   // ... of which in filters beyond the LDS budget
    uint32_t terms;            // distinct terms of the kind in the batch
    uint32_t max_k;            // largest k of the kind's filters in the group
};
inline bool launch_gathers(const GatherKind *kinds, uint32_t n_kinds, uint64_t n_blocks, bool many_terms, uint32_t gather_cost)
{
    if (many_terms || n_kinds == 0 || n_blocks == 0) return false;
    for (uint32_t y = 0; y < n_kinds; ++y) {
        if (kinds[y].unstaged_words != 0 && gather_cost != 0) return false;
        constexpr unsigned __int128 kCap = (unsigned __int128)1 << 80;       // far above any byte count (sum_words x 8 < 2^67): saturating there decides the same
        unsigned __int128 probes = (unsigned __int128)kinds[y].terms * kinds[y].max_k;                       // < 2^64
        probes = probes > kCap / n_blocks ? kCap : probes * n_blocks;
        if (!(probes * gather_cost < (unsigned __int128)kinds[y].sum_words * 8)) return false;               // <= 2^112: no overflow
    }
    return true;
}

// Bytes a gathered launch moves for one kind, as the counters show them (an L2 miss fills a 128-byte line, FETCH_SIZE of
// profiles/probe_gather_lab.txt): a filter of L lines tested at t uniformly spread bits has L (1 - exp(-t / L)) of its lines touched
// in expectation.  L is the kind's mean over the group's blocks; never more than the filters themselves.
// gathered_bytes: t = terms x k, every location of every term — all the host can know before the launch (C2: 275 lines, 290 tests,
// 179 lines).  The gather kernels stop a term at the first phase that finds a clear bit, so they execute fewer tests wherever a term
// is absent from a block (C2: 204.8 tests, 144.5 lines against 159-161 requests per block by the counters); a timestamped launch
// counts the tests it executed on the device, and bsg_timing.stream_bytes is gathered_bytes_tests of that count
// (`tests`: the executed bit tests of the kind summed over the group's blocks).
inline uint64_t gathered_bytes_per_block_tests(const GatherKind &k, uint64_t n_blocks, double tests);
inline uint64_t gathered_bytes(const GatherKind &k, uint64_t n_blocks)
{
    return gathered_bytes_per_block_tests(k, n_blocks, (double)k.terms * (double)k.max_k);
}
inline uint64_t gathered_bytes_tests(const GatherKind &k, uint64_t n_blocks, uint64_t tests)
{
    return n_blocks == 0 ? 0 : gathered_bytes_per_block_tests(k, n_blocks, (double)tests / (double)n_blocks);
}
inline uint64_t gathered_bytes_per_block_tests(const GatherKind &k, uint64_t n_blocks, double tests)
{
    if (n_blocks == 0 || k.sum_words == 0) return 0;
    const double lines = (double)k.sum_words * 8.0 / 128.0 / (double)n_blocks;
    const double touched = lines * (1.0 - std::exp(-tests / lines)) * 128.0 * (double)n_blocks;
    const double all = (double)k.sum_words * 8.0;
    return (uint64_t)(touched < all ? touched : all);
}

// Workgroups of the gather kernels per CU.  The kernels hold no LDS and 8 waves a workgroup, so 4 workgroups share a CU (8 waves per
// SIMD) unless the launch asks for dynamic LDS it never touches: a pad of floor(160 KiB / n) keeps n workgroups there and no more
// (4 / 3 / 2 / 1 workgroups = 8 / 6 / 4 / 2 waves per SIMD).  The pad is rounded DOWN to the LDS allocation unit, so that what the
// hardware rounds up is the pad itself and n workgroups still fit; one workgroup per CU takes the largest request the library
// makes anywhere (kLdsBudget's 144 KiB: two of them do not fit).  Pads above 64 KiB are opt-in per kernel (bsg_open sets the
// attribute for gather_lds_pad(1)).  0, and anything above 4, is "no cap": no pad.
// kGatherWorkgroupsPerCu is the planner's rule (bsg_set_lab key 28 = 0); measured: profiles/probe_gather_lines_lab.txt.
constexpr uint32_t kCuLdsBytes = 160u * 1024u;
constexpr uint32_t kLdsAllocUnit = 1280u;               // gfx950 allocates LDS in units of 320 dwords
constexpr uint32_t kLdsOptInBytes = 64u * 1024u;        // more dynamic LDS than this needs hipFuncAttributeMaxDynamicSharedMemorySize
constexpr uint32_t kGatherPadMax = 144u * 1024u;
constexpr uint32_t kGatherMaxWorkgroupsPerCu = 4;
constexpr uint32_t kGatherWorkgroupsPerCu = 0;
inline uint32_t gather_lds_pad(uint32_t workgroups_per_cu)
{
    if (workgroups_per_cu == 0 || workgroups_per_cu > kGatherMaxWorkgroupsPerCu) return 0;
    return std::min(kCuLdsBytes / workgroups_per_cu / kLdsAllocUnit * kLdsAllocUnit, kGatherPadMax);
}

// Tail split (lab key 19, percent): a run of ONE group of n_shards shards is cut into two dispatches' worth, the first n0 shards
// and the rest.  Returns n0 (1 <= n0 <= n_shards - 1), or 0 where the run is not cut: fewer than 8 shards, or more than one
// launch's kernel arguments hold.
inline size_t tail_split_cut(size_t n_shards, uint32_t pct, size_t max_group_arenas)
{
    if (pct == 0 || n_shards < 8 || n_shards > max_group_arenas) return 0;
    return std::min(n_shards - 1, std::max<size_t>(1, n_shards * pct / 100));
}

// Chunked gather (k_gather_fused): a group that gathers is probed in a few CHUNKS of consecutive arenas on one stream —
//   k_probe_gather(chunk 0) | k_gather_fused(gather chunk i, evaluate chunk i - 1) ... | k_eval_programs(last chunk)
// so that only the last chunk's program evaluation is left behind the probe.  Every further dispatch costs a boundary of a few
// microseconds, so a run is chunked only where the evaluation it hides is longer than that: kPipelineMinArenas arenas AND
// kPipelineMinBlocks blocks (the evaluation's time goes with the 64-block groups, the boundary's does not: many tiny arenas are
// no reason to chunk).  Measured on MI355X with C2's 1 000-block arenas (profiles/probe_pipeline_lab.txt): three equal chunks with
// the evaluation workgroups SPREAD through k_gather_fused's grid take 700 us against 741-745 at 200 arenas and 534 against 560-568 at
// 150; at 50-100 arenas the result depends on what the calls alternate with (a draw against the plain route run by itself), at
// 30 and 20 every chunking loses 3-25 %; with the evaluation workgroups in FRONT of the grid no chunking gains at any size.  So the
// rule starts where a group's records lie in device memory anyway.
// One chunk — the two plain dispatches — whenever the launch does not gather, the batch is not a few-term batch with the identity
// word list, the run has more than one group, or fold / fuse / tail split is selected.
// key (bsg_set_lab key 27): 0 = the rule above; 1 = never; low 16 bits n >= 2 = n chunks (at most one per arena) whatever the
// thresholds say, as equal as possible; bits 16-23 = percent of an equal share the LAST chunk gets (0 = 100: equal) — it is the only
// one whose evaluation stays exposed; bits 24-25 = where k_gather_fused's evaluation workgroups go (0 = kPipelineSpread, 1 = in front,
// 2 = spread among the gather workgroups: not the planner's business).
constexpr uint32_t kPipelineMinArenas = 129;
constexpr uint64_t kPipelineMinBlocks = 128000;
constexpr uint32_t kPipelineChunks = 3;
constexpr uint32_t kPipelineLastPct = 100;
constexpr bool kPipelineSpread = true;
struct PipelineCase {
    bool gathers;          // bsh::launch_gathers of the whole group
    bool identity_few;     // few-term batch with the identity word list
    uint32_t n_groups;     // groups of the run on this device
    bool other_route;      // fold, fuse or tail split selected
};
inline std::vector<uint32_t> pipeline_chunks(uint32_t n_arenas, uint64_t n_blocks, const PipelineCase &pc, uint64_t key)
{
    std::vector<uint32_t> one(n_arenas ? 1 : 0, n_arenas);
    if (n_arenas < 2 || key == 1 || !pc.gathers || !pc.identity_few || pc.n_groups != 1 || pc.other_route) return one;
    uint32_t n = (uint32_t)(key & 0xFFFFu), last_pct = (uint32_t)std::min<uint64_t>((key >> 16) & 0xFFu, 100);
    if (n < 2) {
        if (n_arenas < kPipelineMinArenas || n_blocks < kPipelineMinBlocks) return one;
        n = kPipelineChunks; last_pct = kPipelineLastPct;
    }
    if (last_pct == 0) last_pct = 100;
    n = std::min(n, n_arenas);
    // the last chunk: last_pct of an equal share, at least one arena; the others share the rest as equally as possible
    const uint32_t last = std::max<uint32_t>(1, (uint32_t)((uint64_t)n_arenas * last_pct / (100ull * n)));
    const uint32_t rest = n_arenas - last, m = n - 1;
    std::vector<uint32_t> sizes(n);
    for (uint32_t i = 0; i < m; ++i) sizes[i] = rest / m + (i < rest % m ? 1u : 0u);
    sizes[m] = last;
    return sizes;
}

// bsg_probe_many_rows on a context of nd devices: device d writes the rows of ITS shards (local block numbers: local l of device d is
// global block l * nd + d) into a slice of its own of the caller's page-locked buffers —
//   headers: out_hdr + d * n_arenas * n_queries, [arena][query]
//   rows   : out_rows + row_base[d], arena i's [n_queries][G(i, d)] slots back to back, G(i, d) = ceil(local blocks of (i, d) / 64)
// (nd == 1: exactly the single-device layout).  bsg_survivor_rows_list merges a (arena, query)'s nd rows into global block order.
struct RowsLayout {
    uint32_t nd = 1, n_arenas = 0, n_queries = 0;
    std::vector<uint64_t> row_base;                 // [nd + 1] first row word of device d's slice
    std::vector<std::vector<uint64_t>> arena_off;   // [nd][n_arenas] arena i's rows inside device d's slice
};

// local_blocks(d, i): the blocks of arena i on device d
template <class BlocksOf>
inline RowsLayout rows_layout(uint32_t nd, uint32_t n_arenas, uint32_t n_queries, BlocksOf &&local_blocks)
{
    RowsLayout L;
    L.nd = nd; L.n_arenas = n_arenas; L.n_queries = n_queries;
    L.row_base.assign(nd + 1, 0);
    L.arena_off.assign(nd, std::vector<uint64_t>(n_arenas, 0));
    for (uint32_t d = 0; d < nd; ++d) {
        uint64_t o = 0;
        for (uint32_t i = 0; i < n_arenas; ++i) {
            L.arena_off[d][i] = o;
            o += (uint64_t)n_queries * words64(local_blocks(d, i));
        }
        L.row_base[d + 1] = L.row_base[d] + o;
    }
    return L;
}

// survivors of device di's shard (local block lb == global block lb * nd + di) -> the caller's global bitset (ORed into it).
// An output word holds, from device di, the local bits lo..hi at the positions p0, p0 + nd, ...: one bit-field extract and
// one parallel deposit (BMI2 pdep) per (word, device) instead of a loop over the set bits — a 10 000-block, 4 096-query
// result has 17 M of them.  Hosts without BMI2 take the loop.
inline void interleave_shard_loop(const uint64_t *part, uint32_t Q, uint32_t n_local, uint32_t di, uint32_t nd, uint64_t *dst, uint64_t Gglobal)
{
    const uint32_t G = (n_local + 63) / 64;
    for (uint32_t q = 0; q < Q; ++q) {
        const uint64_t *row = part + (size_t)q * G;
        uint64_t *o = dst + (size_t)q * Gglobal;
        for (uint32_t g = 0; g < G; ++g) {
            uint64_t w = row[g];
            while (w) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(w);
                w &= w - 1;
                const uint64_t b = ((uint64_t)g * 64 + bit) * nd + di;
                o[b >> 6] |= 1ULL << (b & 63);
            }
        }
    }
}

__attribute__((target("bmi2"))) inline void interleave_shard_pdep(const uint64_t *part, uint32_t Q, uint32_t n_local, uint32_t di, uint32_t nd,
                                                                   uint64_t *dst, uint64_t Gglobal)
{
    const uint32_t G = (n_local + 63) / 64;
    // deposit masks by first position p0 < nd: bits p0, p0 + nd, ... below 64
    std::vector<uint64_t> masks(nd, 0);
    for (uint32_t p0 = 0; p0 < nd; ++p0)
        for (uint32_t p = p0; p < 64; p += nd) masks[p0] |= 1ULL << p;
    const uint64_t n_global = (uint64_t)(n_local - 1) * nd + di + 1;      // one past this shard's last global block
    const uint64_t n_words = (n_global + 63) / 64;
    // per output word: first local bit and first position (the same for every query)
    std::vector<uint32_t> lo_of(n_words), p0_of(n_words);
    for (uint64_t ow = 0; ow < n_words; ++ow) {
        const uint64_t first = ow * 64;                                   // lo = ceil((first - di) / nd), clamped at 0
        const uint64_t lo = first > di ? (first - di + nd - 1) / nd : 0;
        lo_of[ow] = (uint32_t)lo;
        p0_of[ow] = (uint32_t)(lo * nd + di - first);
    }
    for (uint32_t q = 0; q < Q; ++q) {
        const uint64_t *row = part + (size_t)q * G;
        uint64_t *o = dst + (size_t)q * Gglobal;
        for (uint64_t ow = 0; ow < n_words; ++ow) {
            const uint32_t lo = lo_of[ow], p0 = p0_of[ow];
            if (lo >= n_local || p0 >= 64) continue;
            const uint32_t wi = lo >> 6, sh = lo & 63u;
            uint64_t src = row[wi] >> sh;
            if (sh && wi + 1 < G) src |= row[wi + 1] << (64 - sh);       // (bits past n_local are zero in the survivors)
            o[ow] |= __builtin_ia32_pdep_di(src, masks[p0]);
        }
    }
}

inline void interleave_shard(const uint64_t *part, uint32_t Q, uint32_t n_local, uint32_t di, uint32_t nd, uint64_t *dst, uint64_t Gglobal)
{
    if (n_local == 0) return;
    static const bool has_bmi2 = __builtin_cpu_supports("bmi2");
    if (has_bmi2 && nd <= 64) interleave_shard_pdep(part, Q, n_local, di, nd, dst, Gglobal);
    else interleave_shard_loop(part, Q, n_local, di, nd, dst, Gglobal);
}

// One device's survivors into the caller's (zeroed) layout: `part` holds the device's non-empty shards back to back in list order,
// shard i as [n_queries][ceil(local_blocks[i] / 64)]; arena i's global bitsets ([n_queries][ceil(global_blocks[i] / 64)]) start at
// dst + out_off[i].
template <class LocalBlocksOf, class GlobalBlocksOf>
inline void merge_device_part(const uint64_t *part, uint32_t n_arenas, LocalBlocksOf &&local_blocks, GlobalBlocksOf &&global_blocks, uint32_t n_queries,
                              uint32_t di, uint32_t nd, uint64_t *dst, const uint64_t *out_off)
{
    uint64_t o = 0;
    for (uint32_t i = 0; i < n_arenas; ++i) {
        const uint32_t n_local = local_blocks(i);
        if (n_local == 0) continue;
        interleave_shard(part + o, n_queries, n_local, di, nd, dst + out_off[i], words64(global_blocks(i)));
        o += (uint64_t)n_queries * words64(n_local);
    }
}

}  // namespace bsh
