// lookup_plan.hpp — the table arithmetic of bsg_match_rows_lookup / bsg_match_rows_lookup_rows (match_api.inc, match_lookup.hip.h), free
// of any device type.  A table of up to kMaxConds Field / Token / FieldToken conditions is resolved per emission by lookup instead of
// by a loop over the conditions:
//   build_strings   the DISTINCT condition strings that play a role (the field of a Field or FieldToken condition, the token of a Token
//                   or FieldToken condition) get ids; per string a role record (the Field condition on it, the Token condition on it,
//                   "is the field of some FieldToken condition", "is the token of some"), per FieldToken condition its (field id,
//                   token id) pair, per condition the first condition equal to it (a repeated condition shares its bit: the programs
//                   are lowered over `canon`)
//   place_strings   the string table: open addressing, linear probing, keyed on word 0 of the string's 256-bit base hash; a slot is a
//                   20-bit tag and a 12-bit id, the full record is read only on a tag hit
//   place_pairs     the pair table: the same probing keyed on (field id, token id); a slot holds the whole key and the condition
//   flag_words / flag_index   W u64 of satisfaction flags per row, stored word-major over the part's rows
// bsg_match_rows_lookup_regex(_rows) adds FieldRegex conditions to such a table (build_strings with regex = true): a regex condition
// takes no role string and no pair, a repeated one (the same field bytes and pattern bytes) shares its first occurrence's bit, the
// first occurrences are the table's regex SLOTS (Plan::rx_conds, the order of the blob host/regex_groups.hpp builds of them), and
//   set_rx_masks    per set of rows one u32: bit j = a program of a query listed on the set references regex slot j
//   lookup_lds_bytes / rx_lds_cap   what the walker's tables and lanes take in LDS, and what that leaves of 80 KiB for the blob
// The slot, tag and probe functions are constexpr: the kernels call the same ones.  tests/lookup_plan_check.cpp runs all of it on the
// CPU (tests/test_match_lookup_plan.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace bsh_lookup {

constexpr uint32_t kMaxConds = 1024;           // bloomgpu.h BSG_MATCH_LOOKUP_MAX_CONDS
constexpr uint32_t kMaxStrings = 2048;         // two per condition
constexpr uint32_t kNoCond = 0xFFFFu, kNoString = 0xFFFFFFFFu;
constexpr uint32_t kIdBits = 12, kIdMask = (1u << kIdBits) - 1u;
constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu;   // id 0xFFF is no string's (ids < kMaxStrings)
constexpr uint64_t kPairEmpty = ~0ull;         // condition 0xFFFFFFFF is no condition's
constexpr uint32_t kKindField = 0, kKindToken = 1, kKindFieldToken = 2, kKindFieldRegex = 3;
constexpr uint32_t kMaxRegexConds = 16;        // host/regex_groups.hpp kMaxRegexConds: one bit of a set's u32 mask each
constexpr uint32_t kRoleFtField = 1u, kRoleFtToken = 2u;
static_assert(kMaxStrings <= kIdMask, "a slot's id field holds every string id and the empty mark");

// ---- role records ----
// entry (the string's first occurrence among the table's 2 * n_conds strings: where its hashes and fingerprint lie) | the Field
// condition on it << 16 | the Token condition on it << 32 | flags << 48
constexpr uint64_t pack_record(uint32_t entry, uint32_t field_cond, uint32_t token_cond, uint32_t flags)
{
    return (uint64_t)entry | (uint64_t)field_cond << 16 | (uint64_t)token_cond << 32 | (uint64_t)flags << 48;
}
constexpr uint32_t rec_entry(uint64_t r) { return (uint32_t)(r & 0xFFFFu); }
constexpr uint32_t rec_field_cond(uint64_t r) { return (uint32_t)(r >> 16) & 0xFFFFu; }
constexpr uint32_t rec_token_cond(uint64_t r) { return (uint32_t)(r >> 32) & 0xFFFFu; }
constexpr uint32_t rec_flags(uint64_t r) { return (uint32_t)(r >> 48); }
// the string is compared with paths / with words
constexpr bool rec_path_role(uint64_t r) { return rec_field_cond(r) != kNoCond || (rec_flags(r) & kRoleFtField) != 0u; }
constexpr bool rec_word_role(uint64_t r) { return rec_token_cond(r) != kNoCond || (rec_flags(r) & kRoleFtToken) != 0u; }

struct Pair {
    uint32_t fid, tid, cond;
};

struct Plan {
    std::vector<uint64_t> rec;             // [n_strings]
    std::vector<uint32_t> string_of;       // [2 * n_conds]: the id of entry e where the condition's kind gives it a role, else kNoString
    std::vector<uint32_t> canon;           // [n_conds]: the first condition with this kind and these role strings
    std::vector<Pair> pairs;               // the distinct FieldToken conditions
    std::vector<uint32_t> rx_conds;        // the distinct FieldRegex conditions, ascending: regex slot j is condition rx_conds[j]
    // the regex slot of condition c (of its first occurrence), or kNoCond where c is no regex condition
    uint32_t rx_slot(uint32_t c) const
    {
        for (uint32_t j = 0; j < rx_conds.size(); ++j)
            if (rx_conds[j] == canon[c]) return j;
        return kNoCond;
    }
    uint32_t n_strings() const { return (uint32_t)rec.size(); }
};

enum class Status { Ok, TooMany, Kind };

// Condition c's strings are entries 2c (field) and 2c + 1 (token) of cond_bytes / cond_off.  Kind: *bad = the first condition that is
// no Field / Token / FieldToken (the call names it in its refusal).  regex: FieldRegex conditions (entry 2c + 1 = the pattern) are
// part of the table too; how many distinct ones a call holds is the blob's limit (regex_groups.hpp), not checked here.
inline Status build_strings(const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds, Plan &pl,
                            uint32_t *bad = nullptr, bool regex = false)
{
    pl = Plan{};
    if (n_conds > kMaxConds) return Status::TooMany;
    for (uint32_t c = 0; c < n_conds; ++c)
        if (cond_kinds[c] > (regex ? kKindFieldRegex : kKindFieldToken)) {
            if (bad) *bad = c;
            return Status::Kind;
        }
    pl.string_of.assign((size_t)2 * n_conds, kNoString);
    pl.canon.resize(n_conds);
    std::unordered_map<std::string, uint32_t> ids;
    std::unordered_map<uint32_t, uint32_t> pair_cond;      // fid << 16 | tid -> condition
    std::unordered_map<std::string, uint32_t> rx_cond;     // field length, field bytes, pattern bytes -> condition
    std::vector<uint32_t> entry, fc, tc, flags;
    auto id_of = [&](uint32_t e) -> uint32_t {
        const std::string s(cond_bytes ? (const char *)cond_bytes + cond_off[e] : "", cond_off[e + 1] - cond_off[e]);
        auto it = ids.emplace(s, (uint32_t)entry.size());
        if (it.second) { entry.push_back(e); fc.push_back(kNoCond); tc.push_back(kNoCond); flags.push_back(0u); }
        return pl.string_of[e] = it.first->second;
    };
    for (uint32_t c = 0; c < n_conds; ++c) {
        const uint32_t kind = cond_kinds[c];
        if (kind == kKindFieldRegex) {                     // no role string, no pair: the walker's DFAs decide it
            const uint32_t flen = cond_off[2 * c + 1] - cond_off[2 * c];
            std::string key((const char *)&flen, 4);
            key.append(cond_bytes ? (const char *)cond_bytes + cond_off[2 * c] : "", cond_off[2 * c + 2] - cond_off[2 * c]);
            auto it = rx_cond.emplace(std::move(key), c);
            if (it.second) pl.rx_conds.push_back(c);
            pl.canon[c] = it.first->second;
            continue;
        }
        const uint32_t f = kind != kKindToken ? id_of(2 * c) : kNoString, t = kind != kKindField ? id_of(2 * c + 1) : kNoString;
        if (kind == kKindField) {
            if (fc[f] == kNoCond) fc[f] = c;
            pl.canon[c] = fc[f];
        } else if (kind == kKindToken) {
            if (tc[t] == kNoCond) tc[t] = c;
            pl.canon[c] = tc[t];
        } else {
            auto it = pair_cond.emplace(f << 16 | t, c);
            if (it.second) { pl.pairs.push_back(Pair{f, t, c}); flags[f] |= kRoleFtField; flags[t] |= kRoleFtToken; }
            pl.canon[c] = it.first->second;
        }
    }
    for (size_t i = 0; i < entry.size(); ++i) pl.rec.push_back(pack_record(entry[i], fc[i], tc[i], flags[i]));
    return Status::Ok;
}

// ---- slot placement and probe sequence ----
// A table of n keys has the least power of two >= 2n slots (at least 2): the load stays <= 1/2 and a probe always meets an empty slot.
constexpr uint32_t table_slots(uint32_t n)
{
    uint32_t s = 2;
    while (s < 2u * n) s <<= 1;
    return s;
}
constexpr uint32_t log2_slots(uint32_t slots)
{
    uint32_t l = 0;
    while ((1u << l) < slots) ++l;
    return l;
}
constexpr uint32_t kMaxStringSlots = table_slots(kMaxStrings), kMaxPairSlots = table_slots(kMaxConds);
static_assert(kMaxStringSlots == 4096u && kMaxPairSlots == 2048u, "match_lookup.hip.h sizes its LDS by these");

// the string table: h0 = word 0 of the base hash.  Slot and tag come from disjoint bits of it.
constexpr uint32_t string_slot0(uint64_t h0, uint32_t slots) { return (uint32_t)h0 & (slots - 1u); }
constexpr uint32_t string_tag(uint64_t h0) { return (uint32_t)(h0 >> 32) & 0xFFFFFu; }
constexpr uint32_t string_slot(uint64_t h0, uint32_t id) { return string_tag(h0) << kIdBits | id; }
constexpr uint32_t next_slot(uint32_t i, uint32_t slots) { return (i + 1u) & (slots - 1u); }

// h0[id] for every string -> the table (table_slots(n) u32).  Strings with equal h0 lie in one probe run: a lookup goes on behind a
// tag hit whose record is not the emission's — and, in the kernel, behind a match too, so that what it finds does not depend on
// the order of placement.
inline std::vector<uint32_t> place_strings(const uint64_t *h0, uint32_t n)
{
    const uint32_t slots = table_slots(n);
    std::vector<uint32_t> tab(slots, kSlotEmpty);
    for (uint32_t id = 0; id < n; ++id) {
        uint32_t i = string_slot0(h0[id], slots);
        while (tab[i] != kSlotEmpty) i = next_slot(i, slots);
        tab[i] = string_slot(h0[id], id);
    }
    return tab;
}

// The candidates of a lookup, in probe order: is(id) says whether string id is the one looked for (the caller compares the full
// record); -> its id or kNoString.  The kernel walks the same sequence.
template <class Is>
inline uint32_t find_string(const uint32_t *tab, uint32_t slots, uint64_t h0, Is &&is)
{
    const uint32_t tag = string_tag(h0);
    uint32_t i = string_slot0(h0, slots);
    for (uint32_t n = 0; n < slots && tab[i] != kSlotEmpty; ++n, i = next_slot(i, slots))
        if ((tab[i] >> kIdBits) == tag && is(tab[i] & kIdMask)) return tab[i] & kIdMask;
    return kNoString;
}

// the pair table: key = (field id, token id), slot = key << 32 | condition
constexpr uint32_t pair_key(uint32_t fid, uint32_t tid) { return fid << 16 | tid; }
constexpr uint32_t pair_shift(uint32_t slots) { return 32u - log2_slots(slots); }      // the host passes it to the kernel
constexpr uint32_t pair_slot0_shift(uint32_t key, uint32_t shift) { return (key * 0x9E3779B1u) >> shift; }
constexpr uint32_t pair_slot0(uint32_t key, uint32_t slots) { return pair_slot0_shift(key, pair_shift(slots)); }

inline std::vector<uint64_t> place_pairs(const std::vector<Pair> &pairs)
{
    const uint32_t slots = table_slots((uint32_t)pairs.size());
    std::vector<uint64_t> tab(slots, kPairEmpty);
    for (const Pair &p : pairs) {
        uint32_t i = pair_slot0(pair_key(p.fid, p.tid), slots);
        while (tab[i] != kPairEmpty) i = next_slot(i, slots);
        tab[i] = (uint64_t)pair_key(p.fid, p.tid) << 32 | p.cond;
    }
    return tab;
}

// -> the FieldToken condition of (fid, tid) or kNoCond
inline uint32_t find_pair(const uint64_t *tab, uint32_t slots, uint32_t fid, uint32_t tid)
{
    const uint32_t key = pair_key(fid, tid);
    uint32_t i = pair_slot0(key, slots);
    for (uint32_t n = 0; n < slots && tab[i] != kPairEmpty; ++n, i = next_slot(i, slots))
        if ((uint32_t)(tab[i] >> 32) == key) return (uint32_t)tab[i];
    return kNoCond;
}

// ---- the regex conditions of a set ----
// One u32 per set: bit j = a program of a query listed on the set references regex slot j (public postfix ops: opcode 0 = TERM, the
// low 28 bits its condition; a repeated condition counts as its first occurrence).  A leaf opens a slot's DFA only on a row whose
// set's mask selects it: bsh_wide::set_cond_masks over slots instead of conditions (a u64 there holds 64 conditions, no 1 024).
inline std::vector<uint32_t> set_rx_masks(const Plan &pl, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                          const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets)
{
    std::vector<uint32_t> slot(pl.canon.size(), kNoCond), query(n_queries, 0u), sets(n_sets, 0u);
    for (uint32_t j = 0; j < pl.rx_conds.size() && j < 32u; ++j) slot[pl.rx_conds[j]] = j;
    for (uint32_t q = 0; q < n_queries; ++q)
        for (uint32_t i = prog_off[q]; i < prog_off[q + 1]; ++i) {
            const uint32_t arg = prog_ops[i] & 0x0FFFFFFFu;
            if ((prog_ops[i] >> 28) == 0u && arg < pl.canon.size() && slot[pl.canon[arg]] != kNoCond) query[q] |= 1u << slot[pl.canon[arg]];
        }
    for (uint32_t s = 0; s < n_sets; ++s)
        for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p)
            if (set_queries[p] < n_queries) sets[s] |= query[set_queries[p]];
    return sets;
}

// ---- LDS ----
// The walker's workgroup: the two tables, then 256 lanes of 116 bytes (ingest.hip.h kIngestThreads * kLaneLds: match_lookup.hip.h
// asserts the product).  The regex walker copies its table blob behind them and keeps two workgroups per CU (160 KiB of LDS), so the
// blob's cap is what the tables of THIS call leave of 80 KiB: 52 200 bytes over an empty plain table, 19 456 over one at its limit.
constexpr uint32_t kLaneBytes = 256u * 116u;
constexpr uint32_t kWorkgroupLds = 80u * 1024u;
constexpr uint32_t lookup_lds_bytes(uint32_t n_str_slots, uint32_t n_pair_slots) { return n_str_slots * 4u + n_pair_slots * 8u + kLaneBytes; }
constexpr uint32_t rx_lds_cap(uint32_t n_str_slots, uint32_t n_pair_slots) { return kWorkgroupLds - lookup_lds_bytes(n_str_slots, n_pair_slots); }
// ... of a table of n_strings role strings and n_pairs FieldToken pairs (upper bounds give a lower bound of the cap)
constexpr uint32_t rx_lds_cap_of(uint32_t n_strings, uint32_t n_pairs) { return rx_lds_cap(table_slots(n_strings), table_slots(n_pairs)); }
static_assert(rx_lds_cap_of(0, 0) == 52200u && rx_lds_cap(kMaxStringSlots, kMaxPairSlots) == 19456u && rx_lds_cap_of(0, 0) < 0x10000u,
              "the regex blob's cap over the empty and the full table; its 16-bit offsets reach every cap");

// ---- the flags ----
// W words per row, word-major over the part's rows: the evaluator's 64 lanes load one word of 64 consecutive rows in one piece.  A
// launch covers rows [row_base, row_base + n) of the part; r counts from row_base.
constexpr uint32_t flag_words(uint32_t n_conds) { return n_conds ? (n_conds + 63u) / 64u : 1u; }
constexpr uint64_t flag_index(uint32_t cond, uint32_t part_rows, uint32_t row_base, uint32_t r)
{
    return (uint64_t)(cond >> 6) * part_rows + row_base + r;
}
constexpr uint64_t flag_bit(uint32_t cond) { return 1ull << (cond & 63u); }
// device memory of the flags and the state byte per row of a part
constexpr uint64_t flag_bytes_per_row(uint32_t n_conds) { return 8ull * flag_words(n_conds) + 1ull; }

}  // namespace bsh_lookup
