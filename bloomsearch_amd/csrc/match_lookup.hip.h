// match_lookup.hip.h — the row matcher over tables of up to 1 024 Field / Token / FieldToken conditions (bsg_match_rows_lookup /
// bsg_match_rows_lookup_rows).  match.hip.h's walkers compare every emission with every table condition, and keep the flags in one
// register: both bound the table at 64 conditions.  Here an emission is resolved by LOOKUP and the flags are W = ceil(n_conds / 64)
// words per row in device memory.
//
// k_match_rows_lookup / _tok, the storing walker: the same resumable walker, one row per lane.  The table's distinct role strings
// (host/lookup_plan.hpp build_strings, at most 2 048) have ids.  LDS holds two open-addressing tables (linear probing, load <= 1/2,
// placed by the host from the hashes k_hash_fp_entries made):
//   strings  u32 slots: 20-bit tag | 12-bit id, keyed on word 0 of the emission's base hash
//   pairs    u64 slots: (field id << 16 | token id) << 32 | condition, keyed on the ids
// An emission probes the string table; only on a tag hit is the string's record read from device memory (hits are rare, the records
// stay in L2): its role word, then the four hash words and the keyed fingerprint of its entry in cond_h / cond_fp.  Equality is
// decided on all four words AND the fingerprint as in match.hip.h; equal words with another fingerprint make the row a fallback row
// when the string has a role for this kind of emission (a path role for field / leaf requests, a word role for words), and the probe
// goes on to the run's empty slot even behind a match (two table strings may share their hashes: the row is then a fallback row wherever
// the two were placed).  A path that is a Field condition's sets that condition's flag; a leaf path
// that is some FieldToken condition's field is kept as the leaf's field id; a word that is a Token condition's sets its flag, and,
// when it is some FieldToken condition's token and the leaf has a field id, probes the pair table for (field id, token id): the pair
// holds at ONE leaf, never across leaves.
// Flags: a lane ORs a hit into its own row's word in device memory, zeroed before the walk (sat[w * part_rows + row], word-major:
// host/lookup_plan.hpp flag_index).  No other lane touches that word, so a plain read-modify-write is enough, and a hit is rare:
// most rows of a search's survivors satisfy a few of a thousand conditions.  A per-lane strip of W words in LDS would cost 32 KiB
// for 256 lanes at W = 16 and be written back whole for every row.
// LDS: strings <= 16 384 + pairs <= 16 384 + lanes 29 696 = 62 464 bytes at most, two workgroups per CU; a launch asks for what its
// tables take.
//
// k_match_rows_lookup_regex / _regex_tok (bsg_match_rows_lookup_regex / _rows), the same body with REGEX = true: the table also holds
// up to kRxMaxConds DISTINCT FieldRegex conditions.  They have no role string and no pair; their DFAs are match.hip.h's table blob
// (host/regex_groups.hpp build_blob_of, the single call's layout without user masks), copied into LDS BEHIND the lanes' region: strings,
// pairs, lanes, blob — the lanes stay where the plain instance has them, and the end of the lanes (a multiple of 8) is 4-byte aligned.
// A lane reads its set's u32 of regex slots once (set_rx_mask, host/lookup_plan.hpp set_rx_masks) beside set_pair_off; the leaf-request
// round is match_rows_body's, wave-uniform, and opens slot j only where bit j of that word is set (the storing walker's rule with the
// slot's bit in place of the condition's); at the row's end every slot that matched is ORed into the row's own flag word, like any
// other hit.  A fifth regex condition on one leaf, among those the row's set selects, makes the row a fallback row.
// LDS: lookup_lds_bytes + the blob's bytes <= 80 KiB, two workgroups per CU: the blob's cap is what THIS call's tables leave
// (bsh_lookup::rx_lds_cap: 52 200 bytes over an empty plain table, 19 456 over one at its limit).
//
// k_eval_row_programs_w: k_eval_row_programs with TERM c reading bit c & 63 of word c >> 6.  The word index is wave-uniform (the
// program is read on the scalar path), the 64 lanes load 64 consecutive u64; the last word loaded is kept.
#pragma once
#include "match.hip.h"
#include "host/lookup_plan.hpp"

namespace bsg {

constexpr uint32_t kLookupMaxConds = bsh_lookup::kMaxConds;
constexpr uint32_t kLookupTabBytes = bsh_lookup::kMaxStringSlots * 4u + bsh_lookup::kMaxPairSlots * 8u;
constexpr uint32_t kMatchLookupLdsBytes = kLookupTabBytes + kIngestThreads * kLaneLds;      // the most a launch asks for
static_assert(kMatchLookupLdsBytes <= 80u * 1024u && 2u * kMatchLookupLdsBytes <= 160u * 1024u, "k_match_rows_lookup keeps two workgroups per CU");
static_assert(bsh_lookup::kLaneBytes == kIngestThreads * kLaneLds && bsh_lookup::kMaxRegexConds == kRxMaxConds, "host/lookup_plan.hpp states the walker's lanes and regex limit");

struct MatchLookupArgs {
    const uint32_t *set_first_row;   // [n_sets + 1], in the rows MatchArgs::row_base counts; n_sets >= 1
    const uint32_t *set_pair_off;    // [n_sets + 1]: an empty range = the set's rows are not walked
    const uint32_t *str_slots;       // [n_str_slots] host/lookup_plan.hpp place_strings
    const uint64_t *pair_slots;      // [n_pair_slots] place_pairs
    const uint64_t *recs;            // [n_strings] pack_record
    uint64_t *sat;                   // the launch's first row of word 0; word w of row r at sat[w * part_rows + r].  Zeroed by the host
    uint8_t *state;                  // [n_rows] of the launch
    uint32_t n_sets, n_str_slots, n_pair_slots, part_rows;
    uint32_t pair_shift;             // host/lookup_plan.hpp pair_shift(n_pair_slots)
    const uint32_t *set_rx_mask;     // [n_sets], the regex walkers only: bit j = the set's queries use regex slot j (set_rx_masks)
};

constexpr uint32_t lookup_lds_bytes(uint32_t n_str_slots, uint32_t n_pair_slots) { return bsh_lookup::lookup_lds_bytes(n_str_slots, n_pair_slots); }
// the regex blob's cap over these tables: with it a workgroup asks for 80 KiB at most, two per CU
constexpr uint32_t lookup_rx_lds_cap(uint32_t n_str_slots, uint32_t n_pair_slots) { return bsh_lookup::rx_lds_cap(n_str_slots, n_pair_slots); }
static_assert(2u * (lookup_lds_bytes(0, 0) + lookup_rx_lds_cap(0, 0)) <= 160u * 1024u &&
                  2u * (kMatchLookupLdsBytes + lookup_rx_lds_cap(bsh_lookup::kMaxStringSlots, bsh_lookup::kMaxPairSlots)) <= 160u * 1024u &&
                  lookup_rx_lds_cap(2, 2) <= 0x10000u,
              "k_match_rows_lookup_regex keeps two workgroups per CU, and the blob's 16-bit offsets reach every cap");

template <bool REGEX, class TOK>
__device__ __forceinline__ void match_rows_lookup_body(const MatchArgs &a, const RxArgs &x, const MatchLookupArgs &lk, const TOK &tk)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    lds_u32 *stab = (lds_u32 *)lds_raw;
    lds_u64i *ptab = (lds_u64i *)(lds_raw + lk.n_str_slots * 4u);
    for (uint32_t i = threadIdx.x; i < lk.n_str_slots; i += kIngestThreads) stab[i] = lk.str_slots[i];
    for (uint32_t i = threadIdx.x; i < lk.n_pair_slots; i += kIngestThreads) ptab[i] = lk.pair_slots[i];
    const uint32_t rx_base = REGEX ? lookup_lds_bytes(lk.n_str_slots, lk.n_pair_slots) : 0u;   // the blob: behind the lanes
    if constexpr (REGEX)
        for (uint32_t i = threadIdx.x; i < x.n_words; i += kIngestThreads) ((lds_u32 *)(lds_raw + rx_base))[i] = x.blob[i];
    __syncthreads();
    const uint32_t r = blockIdx.x * kIngestThreads + threadIdx.x;
    const bool live = r < a.n_rows;
    Walker w;
    ChunkCursor cc;
    walker_bind(w, cc, a.rows, (lds_u8 *)lds_raw + lk.n_str_slots * 4u + lk.n_pair_slots * 8u + threadIdx.x * kLaneLds, a.lower, a.key, false);
    bool listed = false;         // the row's set has a pair at all
    uint32_t smask = 0;          // REGEX: the regex slots the set's queries use
    if (live) {
        const uint32_t lo = row_set_of(lk.set_first_row, lk.n_sets, a.row_base + r);
        listed = lk.set_pair_off[lo + 1] != lk.set_pair_off[lo];
        if constexpr (REGEX) smask = lk.set_rx_mask[lo];
    }
    const bool walk = listed;
    walker_reset(w, cc, walk ? a.row_off[r] : 0, walk ? a.row_off[r + 1] : 0, walk);
    uint32_t res = walk ? R_CONTINUE : R_DONE;
    uint32_t leaf_fid = bsh_lookup::kNoString;   // the current leaf's path as a FieldToken field
    bool collided = false;       // equal hashes, different fingerprint: only the host's byte compare can decide this row
    typename std::conditional<REGEX, RxLane, RxNone>::type rx;
    bool rx_over = false;        // more regex conditions on one leaf than a lane holds: the host decides this row
    if constexpr (REGEX) {
        rx.tab = (const lds_u8 *)lds_raw + rx_base;
        rx.sat = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRxActive; ++k) rx.hd[k] = ~0u;
    }
    uint64_t *my_sat = lk.sat + r;               // word w of this lane's row: my_sat[w * part_rows]
    while (__ballot(res == R_CONTINUE || w.req != Q_NONE) != 0ull) {
        while (__ballot(res == R_CONTINUE && w.req == Q_NONE) != 0ull)
            if (res == R_CONTINUE && w.req == Q_NONE) res = advance<true>(w, cc, rx, tk);
        const uint32_t q = w.req;
        w.req = Q_NONE;
        HashStream s;
        hs_init(s, w.key);
        const uint32_t plen = (q == Q_FIELD || q == Q_LEAF) ? w.req_len : 0u;
        for (uint32_t i = 0; __ballot(i < plen) != 0ull; ++i)
            if (i < plen) hs_absorb(s, w.path[i], w.key);
        if (q == Q_WORD) { word_request<TOK>(w); s = w.tok; }
        uint64_t h[4] = {0, 0, 0, 0}, fp = 0;
        if (q != Q_NONE) fp = hs_finish(s, h, w.key);
        if (q == Q_LEAF) leaf_fid = bsh_lookup::kNoString;
        if constexpr (REGEX) {                                               // match_rows_body's leaf-request round
            if (q == Q_LEAF) rx.close();                                     // the previous leaf's text ended before this request
            const bool text = q == Q_LEAF && !(w.st == S_LIT && w.lit == 2u);   // null is never a candidate text
            const lds_u32 *hdr = (const lds_u32 *)rx.tab;
            for (uint32_t j = 0; j < x.n_rx && __ballot(text) != 0ull; ++j) {   // uniform loop: header words are LDS broadcasts
                const uint32_t h0 = hdr[4 * j], h1 = hdr[4 * j + 1], h2 = hdr[4 * j + 2], flen = h2 >> 16;
                const lds_u8 *fld = rx.tab + (h2 & 0xFFFFu);
                bool under = text && !((rx.sat >> j) & 1u) && flen != 0u && flen <= kPathCap &&
                             (plen == flen || (plen > flen && w.path[flen] == '.')) && ((smask >> j) & 1u) != 0u;   // ... whose set lists a query that uses it
                for (uint32_t i = 0; i < flen && __ballot(under) != 0ull; ++i)   // ends once no lane's path can still match
                    if (under) under = w.path[i] == fld[i];
                if (under) {
                    const uint32_t sv = h1 & 0xFFFFu;
                    if (sv & kRxAccept) rx.sat |= 1u << j;                   // the pattern matches every text (an empty match)
                    else if (!(sv & kRxDead)) {
                        bool placed = false;
#pragma unroll
                        for (uint32_t k = 0; k < kRxActive; ++k)
                            if (!placed && rx.hd[k] == ~0u) { rx.hd[k] = h0; rx.st[k] = sv; placed = true; }
                        rx_over |= !placed;
                    }
                }
            }
        }
        if (q != Q_NONE) {
            const bool is_path = q != Q_WORD;
            const uint32_t tag = bsh_lookup::string_tag(h[0]);
            uint32_t i = bsh_lookup::string_slot0(h[0], lk.n_str_slots);
            for (uint32_t n = 0; n < lk.n_str_slots; ++n, i = bsh_lookup::next_slot(i, lk.n_str_slots)) {   // ends at an empty slot: the load is <= 1/2
                const uint32_t slot = stab[i];
                if (slot == bsh_lookup::kSlotEmpty) break;
                if ((slot >> bsh_lookup::kIdBits) != tag) continue;
                const uint32_t id = slot & bsh_lookup::kIdMask;
                const uint64_t rec = lk.recs[id];
                const uint32_t e = bsh_lookup::rec_entry(rec);
                const uint64_t *eh = a.cond_h + (uint64_t)e * 4u;
                if (eh[0] != h[0] || eh[1] != h[1] || eh[2] != h[2] || eh[3] != h[3]) continue;
                if (!(is_path ? bsh_lookup::rec_path_role(rec) : bsh_lookup::rec_word_role(rec))) continue;   // not compared with this kind of emission
                if (a.cond_fp[e] != fp) { collided = true; continue; }
                const uint32_t c = is_path ? bsh_lookup::rec_field_cond(rec) : bsh_lookup::rec_token_cond(rec);
                if (c != bsh_lookup::kNoCond)                                                    // Field: any emission of that path; Token: anywhere
                    my_sat[(uint64_t)(c >> 6) * lk.part_rows] |= bsh_lookup::flag_bit(c);
                if (q == Q_LEAF && (bsh_lookup::rec_flags(rec) & bsh_lookup::kRoleFtField)) leaf_fid = id;    // this leaf's words may complete a pair
                if (q == Q_WORD && (bsh_lookup::rec_flags(rec) & bsh_lookup::kRoleFtToken) && leaf_fid != bsh_lookup::kNoString) {
                    const uint32_t key = bsh_lookup::pair_key(leaf_fid, id);
                    uint32_t j = bsh_lookup::pair_slot0_shift(key, lk.pair_shift);
                    for (uint32_t m = 0; m < lk.n_pair_slots; ++m, j = bsh_lookup::next_slot(j, lk.n_pair_slots)) {
                        const uint64_t ps = ptab[j];
                        if (ps == bsh_lookup::kPairEmpty) break;
                        if ((uint32_t)(ps >> 32) == key) {
                            const uint32_t pc = (uint32_t)ps;
                            my_sat[(uint64_t)(pc >> 6) * lk.part_rows] |= bsh_lookup::flag_bit(pc);
                            break;
                        }
                    }
                }
                // no break: another table string may share all four hash words (its fingerprint then differs: a fallback row,
                // wherever the two lie in the probe run, as in match.hip.h's loop over every condition)
            }
        }
    }
    if constexpr (REGEX) {
        // the slots that matched, each ORed into the row's own word of its condition (header word 1): hits only, <= kRxMaxConds
        rx.close();
        const lds_u32 *hdr = (const lds_u32 *)rx.tab;
        for (uint32_t j = 0; j < x.n_rx; ++j)
            if ((rx.sat >> j) & 1u) {
                const uint32_t c = hdr[4 * j + 1] >> 16;
                my_sat[(uint64_t)(c >> 6) * lk.part_rows] |= bsh_lookup::flag_bit(c);
            }
        if (rx_over && res == R_DONE) res = R_FAIL;
    }
    if (collided && res == R_DONE) res = R_FAIL;
    if (live) lk.state[r] = !walk ? kRowNotWalked : res == R_DONE ? kRowDecided : kRowFallback;
    if (res == R_FAIL) report_fallback(a, a.row_base + r);
}

// dynamic LDS: lookup_lds_bytes(n_str_slots, n_pair_slots) <= kMatchLookupLdsBytes
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup(const MatchArgs a, const MatchLookupArgs lk)
{
    match_rows_lookup_body<false>(a, RxArgs{}, lk, TokDefault{});
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_tok(const MatchArgs a, const MatchLookupArgs lk, const TokSpec t)
{
    match_rows_lookup_body<false>(a, RxArgs{}, lk, TokSpecP{t});
}
// the table also holds FieldRegex conditions; dynamic LDS: lookup_lds_bytes(...) + the table blob (<= lookup_rx_lds_cap(...))
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_regex(const MatchArgs a, const RxArgs x, const MatchLookupArgs lk)
{
    match_rows_lookup_body<true>(a, x, lk, TokDefault{});
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_regex_tok(const MatchArgs a, const RxArgs x, const MatchLookupArgs lk, const TokSpec t)
{
    match_rows_lookup_body<true>(a, x, lk, TokSpecP{t});
}
// the same two under a spec with an n-gram width (TokGramP)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_gram(const MatchArgs a, const MatchLookupArgs lk, const TokSpec t)
{
    match_rows_lookup_body<false>(a, RxArgs{}, lk, TokGramP(t));
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_regex_gram(const MatchArgs a, const RxArgs x, const MatchLookupArgs lk, const TokSpec t)
{
    match_rows_lookup_body<true>(a, x, lk, TokGramP(t));
}

// k_eval_row_programs over W flag words per row (word-major over the part's part_rows rows).  Items, pairs, programs: RowEvalArgs.
struct RowEvalWArgs {
    RowEvalArgs e;
    uint32_t part_rows;
};
// TERM c reads bit c & 63 of word c >> 6 of the lane's row; the last word loaded is kept (the word index is wave-uniform)
struct SatWords {
    const uint64_t *my_sat;
    uint32_t part_rows;
    bool live;
    uint32_t cur = ~0u;
    uint64_t sat = 0;
    __device__ __forceinline__ uint64_t operator()(uint32_t c)
    {
        if ((c >> 6) != cur) {
            cur = c >> 6;
            sat = live ? my_sat[(uint64_t)cur * part_rows] : 0ull;
        }
        return (sat >> (c & 63u)) & 1ULL;
    }
};
__global__ __launch_bounds__(kRowEvalThreads) void k_eval_row_programs_w(const RowEvalWArgs a)
{
    eval_row_programs_body(a.e, [&](uint32_t row, bool live) { return SatWords{a.e.sat + row, a.part_rows, live}; });
}

}  // namespace bsg
