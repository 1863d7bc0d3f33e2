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
};

constexpr uint32_t lookup_lds_bytes(uint32_t n_str_slots, uint32_t n_pair_slots)
{
    return n_str_slots * 4u + n_pair_slots * 8u + kIngestThreads * kLaneLds;
}

template <class TOK>
__device__ __forceinline__ void match_rows_lookup_body(const MatchArgs &a, const MatchLookupArgs &lk, const TOK &tk)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    lds_u32 *stab = (lds_u32 *)lds_raw;
    lds_u64i *ptab = (lds_u64i *)(lds_raw + lk.n_str_slots * 4u);
    for (uint32_t i = threadIdx.x; i < lk.n_str_slots; i += kIngestThreads) stab[i] = lk.str_slots[i];
    for (uint32_t i = threadIdx.x; i < lk.n_pair_slots; i += kIngestThreads) ptab[i] = lk.pair_slots[i];
    __syncthreads();
    const uint32_t r = blockIdx.x * kIngestThreads + threadIdx.x;
    const bool live = r < a.n_rows;
    Walker w;
    ChunkCursor cc;
    walker_bind(w, cc, a.rows, (lds_u8 *)lds_raw + lk.n_str_slots * 4u + lk.n_pair_slots * 8u + threadIdx.x * kLaneLds, a.lower, a.key, false);
    bool listed = false;         // the row's set has a pair at all
    if (live) {
        const uint32_t lo = row_set_of(lk.set_first_row, lk.n_sets, a.row_base + r);
        listed = lk.set_pair_off[lo + 1] != lk.set_pair_off[lo];
    }
    const bool walk = listed;
    walker_reset(w, cc, walk ? a.row_off[r] : 0, walk ? a.row_off[r + 1] : 0, walk);
    uint32_t res = walk ? R_CONTINUE : R_DONE;
    uint32_t leaf_fid = bsh_lookup::kNoString;   // the current leaf's path as a FieldToken field
    bool collided = false;       // equal hashes, different fingerprint: only the host's byte compare can decide this row
    RxNone rx;
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
        if (q == Q_WORD) s = w.tok;
        uint64_t h[4] = {0, 0, 0, 0}, fp = 0;
        if (q != Q_NONE) fp = hs_finish(s, h, w.key);
        if (q == Q_LEAF) leaf_fid = bsh_lookup::kNoString;
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
    if (collided && res == R_DONE) res = R_FAIL;
    if (live) lk.state[r] = !walk ? kRowNotWalked : res == R_DONE ? kRowDecided : kRowFallback;
    if (res == R_FAIL) report_fallback(a, a.row_base + r);
}

// dynamic LDS: lookup_lds_bytes(n_str_slots, n_pair_slots) <= kMatchLookupLdsBytes
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup(const MatchArgs a, const MatchLookupArgs lk)
{
    match_rows_lookup_body(a, lk, TokDefault{});
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_lookup_tok(const MatchArgs a, const MatchLookupArgs lk, const TokSpec t)
{
    match_rows_lookup_body(a, lk, TokSpecP{t});
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
