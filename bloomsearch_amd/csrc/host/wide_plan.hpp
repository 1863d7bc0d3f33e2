// wide_plan.hpp — the arithmetic of the row-matcher calls (match_api.inc), free of any device type.  For every call: where its rows are
// cut between devices (part_cuts: at set-relative multiples of 64 rows, so no two devices write one word; the single and batched calls
// pass one implicit set {0, n_rows} and get multiples of 64 rows) and the sets a part's rows lie in (part_set_range).  For
// bsg_match_rows_wide: where a (set, query) pair's bit row lies in the result (pair_words), which conditions a set's queries reference
// (query_cond_masks / set_cond_masks: the mask the storing walker opens a regex condition's DFA by), a part's pairs and tiles
// (part_sets) and the work items of k_eval_row_programs (eval_items: a wave owns 64 consecutive rows of ONE set and a range of its
// pairs).  tests/wide_plan_check.cpp runs the same code on the CPU (tests/test_match_wide_plan.py).  For bsg_match_rows_wide_rows: a
// pair's tag and header (pair_tag / pair_header), a header's payload size, offsets from headers, bsg_match_pair_rows_list's
// expansion, the stitch of a multi-device call (stitch_headers / stitch_payloads) and the set table of the device's list passes
// (pair_sets); tests/wide_rows_check.cpp runs those (tests/test_match_wide_rows_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsh_wide {

constexpr uint32_t kMaxQueries = 1u << 20;     // bloomgpu.h bsg_match_rows_wide: queries of one call
constexpr uint32_t kMaxOps = 1u << 22;         // lowered ops of all programs together (16 MiB of device scratch)
constexpr uint32_t kMaxPairs = 1u << 24;       // (set, query) pairs of one call
constexpr uint32_t kMaxItems = 1u << 30;       // work items of one device's evaluation launch
constexpr uint32_t kItemPairs = 64;            // pairs one wave evaluates over its 64 rows
constexpr uint32_t kWideLdsCap = 46592;        // match.hip.h kRxWideLdsCap: regex table bytes of the storing walker

inline uint32_t tiles_of(uint32_t n_rows) { return n_rows / 64u + (n_rows % 64u ? 1u : 0u); }

enum class SizeStatus { Ok, Null, SetSpan, SetOrder, PairOrder };

// Pair p of set s owns tiles_of(rows of s) consecutive words, pairs in order: pair_word_off [n_pairs + 1] (may be NULL) and the
// total.  set_first_row == NULL && set_query_off == NULL && n_sets == 0: one implicit set of all rows with every query.
inline SizeStatus pair_words(const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets, uint32_t n_rows, uint32_t n_queries,
                             uint64_t *pair_word_off, uint64_t *total_words, uint32_t *bad_set = nullptr)
{
    uint64_t at = 0;
    if (n_sets == 0) {
        if (set_first_row || set_query_off) return SizeStatus::Null;
        for (uint32_t q = 0; q < n_queries; ++q) {
            if (pair_word_off) pair_word_off[q] = at;
            at += tiles_of(n_rows);
        }
        if (pair_word_off) pair_word_off[n_queries] = at;
        if (total_words) *total_words = at;
        return SizeStatus::Ok;
    }
    if (!set_first_row || !set_query_off) return SizeStatus::Null;
    if (set_first_row[0] != 0 || set_first_row[n_sets] != n_rows) return SizeStatus::SetSpan;
    for (uint32_t s = 0; s < n_sets; ++s) {
        if (bad_set) *bad_set = s;
        if (set_first_row[s + 1] < set_first_row[s]) return SizeStatus::SetOrder;
        if (set_query_off[s + 1] < set_query_off[s] || (s == 0 && set_query_off[0] != 0)) return SizeStatus::PairOrder;
    }
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t t = tiles_of(set_first_row[s + 1] - set_first_row[s]);
        for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) {
            if (pair_word_off) pair_word_off[p] = at;
            at += t;
        }
    }
    if (pair_word_off) pair_word_off[set_query_off[n_sets]] = at;
    if (total_words) *total_words = at;
    return SizeStatus::Ok;
}

// bit c of masks[q]: program q references condition c (public postfix ops: opcode 0 = TERM, the low 28 bits its condition)
inline std::vector<uint64_t> query_cond_masks(const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, uint32_t n_conds)
{
    std::vector<uint64_t> masks(n_queries, 0);
    for (uint32_t q = 0; q < n_queries; ++q)
        for (uint32_t j = prog_off[q]; j < prog_off[q + 1]; ++j) {
            const uint32_t arg = prog_ops[j] & 0x0FFFFFFFu;
            if ((prog_ops[j] >> 28) == 0u && arg < n_conds && arg < 64u) masks[q] |= 1ull << arg;
        }
    return masks;
}

// per set: the OR of its listed queries' masks.  A set with pairs and mask 0 (only constant programs) is still walked: what says
// "not walked" is an empty list, not an empty mask.
inline std::vector<uint64_t> set_cond_masks(const std::vector<uint64_t> &query_masks, const uint32_t *set_query_off, const uint32_t *set_queries,
                                            uint32_t n_sets)
{
    std::vector<uint64_t> masks(n_sets, 0);
    for (uint32_t s = 0; s < n_sets; ++s)
        for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) masks[s] |= query_masks[set_queries[p]];
    return masks;
}

// Cut points of a call's rows for `want` devices of about equal bytes: each cut lies at a set-relative multiple of 64 rows (a
// whole number of the set's 64-row tiles before it), so every (pair, tile) word is written by one device.  [0, ..., n_rows].
// A target inside the last row counts as a row of the last set: the cut is that set's last tile boundary.
inline std::vector<uint32_t> part_cuts(const uint64_t *row_off, uint32_t n_rows, const uint32_t *set_first_row, uint32_t n_sets, uint32_t want)
{
    std::vector<uint32_t> cuts{0};
    const uint64_t n_bytes = row_off[n_rows] - row_off[0];
    for (uint32_t i = 1; i < want; ++i) {
        const uint64_t target = row_off[0] + n_bytes * i / want;
        uint32_t r = (uint32_t)(std::lower_bound(row_off, row_off + n_rows, target) - row_off);
        // the set r lies in: the last one that begins at or before it
        const uint32_t s = (uint32_t)(std::upper_bound(set_first_row, set_first_row + n_sets, r) - set_first_row) - 1u;
        r = set_first_row[s] + (r - set_first_row[s]) / 64u * 64u;
        if (r > cuts.back() && r < n_rows) cuts.push_back(r);
    }
    cuts.push_back(n_rows);
    return cuts;
}

// The sets rows [r0, r1) of a call lie in, s0 on, their first rows clamped to the part and counted from r0 (what a walker's set
// search reads; the batched call needs no more).
struct SetRange {
    uint32_t s0 = 0;                       // the call's set of local set 0
    std::vector<uint32_t> first_row;       // [n + 1], counted from r0
    uint32_t n() const { return (uint32_t)first_row.size() - 1u; }
};

inline SetRange part_set_range(const uint32_t *set_first_row, uint32_t n_sets, uint32_t r0, uint32_t r1)
{
    SetRange sr;
    const uint32_t *sf = set_first_row;
    sr.s0 = (uint32_t)(std::upper_bound(sf + 1, sf + n_sets + 1, r0) - (sf + 1));            // the first set that ends behind r0
    const uint32_t s1 = (uint32_t)(std::lower_bound(sf, sf + n_sets, r1) - sf);              // the first set that begins at or behind r1
    for (uint32_t s = sr.s0; s < s1; ++s) sr.first_row.push_back(std::max(sf[s], r0) - r0);
    sr.first_row.push_back(r1 - r0);
    return sr;
}

// ... and, for the wide call, per local set its pairs (indices into the call's set_queries) and the set's tile its first row begins
// (r0 is a set-relative multiple of 64).
struct PartSets : SetRange {
    std::vector<uint32_t> pair_off;        // [n + 1] into the call's set_queries
    std::vector<uint32_t> tile0;           // [n]: local tile 0 is this tile of the call's set
};

inline PartSets part_sets(const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets, uint32_t r0, uint32_t r1)
{
    PartSets ps;
    static_cast<SetRange &>(ps) = part_set_range(set_first_row, n_sets, r0, r1);
    for (uint32_t ls = 0; ls < ps.n(); ++ls) {
        ps.pair_off.push_back(set_query_off[ps.s0 + ls]);
        ps.tile0.push_back((ps.first_row[ls] + r0 - set_first_row[ps.s0 + ls]) / 64u);
    }
    ps.pair_off.push_back(set_query_off[ps.s0 + ps.n()]);
    return ps;
}

// One wave of k_eval_row_programs: rows [row0, row0 + n_rows) of the part (n_rows <= 64, one tile of one set), pairs [pair0, pair1)
// of the part's pair list, and where pair0's word goes in the part's result; the next pair's word lies `stride` words on (the
// part's tiles of the set).
struct EvalItem {
    uint64_t out0;
    uint32_t row0, n_rows, pair0, pair1, stride, pad;
};
static_assert(sizeof(EvalItem) == 32, "k_eval_row_programs reads an item as four u64");

// The part's result: local pair lp of local set ls owns tiles_of(local rows) words, pairs in order (for a part that holds its sets
// whole, the call's layout from its first pair on).  pair_off_local counts from the part's first pair.  false: over kMaxItems.
inline bool eval_items(const PartSets &ps, std::vector<EvalItem> &items, uint64_t &part_words)
{
    items.clear();
    uint64_t at = 0;
    for (uint32_t ls = 0; ls < ps.n(); ++ls) {
        const uint32_t rows = ps.first_row[ls + 1] - ps.first_row[ls], tiles = tiles_of(rows);
        const uint32_t p0 = ps.pair_off[ls] - ps.pair_off[0], p1 = ps.pair_off[ls + 1] - ps.pair_off[0];
        if (p0 == p1 || tiles == 0) continue;
        if ((uint64_t)tiles * ((p1 - p0 + kItemPairs - 1) / kItemPairs) + items.size() > kMaxItems) return false;
        for (uint32_t pa = p0; pa < p1; pa += kItemPairs)
            for (uint32_t t = 0; t < tiles; ++t)
                items.push_back(EvalItem{at + (uint64_t)(pa - p0) * tiles + t, ps.first_row[ls] + t * 64u, std::min(64u, rows - t * 64u), pa,
                                         std::min(p1, pa + kItemPairs), tiles, 0u});
        at += (uint64_t)tiles * (p1 - p0);
    }
    part_words = at;
    return true;
}

// ---- bsg_match_rows_wide_rows: a pair's matches as a tagged row list ----
// Header = tag << 30 | n.  c of the pair's R rows match, T = tiles_of(R): NONE c == 0; ALL c == R > 0; LIST 0 < c < R and c < 2T, n = c
// and c ascending set-relative row indices; DENSE otherwise, the pair's T words as 2T u32 (low half first).  The tag is a function
// of (c, R) alone, and no payload is longer than the pair's bit row.  match.hip.h states the same rule for the device.
constexpr uint32_t kPairNone = 0, kPairAll = 1, kPairList = 2, kPairDense = 3;
constexpr uint32_t kPairScanWidth = 256;       // pairs one workgroup of the device's offset scan covers (BSG_MATCH_PAIR_SCAN_WIDTH)

inline uint32_t pair_tag(uint64_t c, uint32_t R)
{
    if (c == 0) return kPairNone;
    if (c == R) return kPairAll;
    return c < 2ull * tiles_of(R) ? kPairList : kPairDense;
}
inline uint32_t pair_header(uint64_t c, uint32_t R)
{
    const uint32_t tag = pair_tag(c, R);
    return tag << 30 | (tag == kPairList ? (uint32_t)c : 0u);
}
// u32 of payload behind a header of a pair over R rows
inline uint64_t pair_payload_size(uint32_t hdr, uint32_t R)
{
    const uint32_t tag = hdr >> 30;
    return tag == kPairList ? (hdr & 0x3FFFFFFFu) : tag == kPairDense ? 2ull * tiles_of(R) : 0ull;
}
// Where each pair's payload begins, from the headers: pair p of set s (pair_off[s] <= p < pair_off[s + 1], rows first_row[s] to
// first_row[s + 1]) has header hdr[p - pair_off[0]] — the call's tables (pair_off[0] == 0) or a part's (PartSets).  off
// [n_pairs + 1] may be NULL; -> the total.
inline uint64_t pair_payload_offsets(const uint32_t *hdr, const uint32_t *first_row, const uint32_t *pair_off, uint32_t n_sets, uint64_t *off)
{
    uint64_t at = 0;
    for (uint32_t s = 0; s < n_sets; ++s)
        for (uint32_t p = pair_off[s]; p < pair_off[s + 1]; ++p) {
            if (off) off[p - pair_off[0]] = at;
            at += pair_payload_size(hdr[p - pair_off[0]], first_row[s + 1] - first_row[s]);
        }
    if (off) off[pair_off[n_sets] - pair_off[0]] = at;
    return at;
}

inline uint64_t dense_word(const uint32_t *payload, uint32_t t) { return payload[2 * t] | (uint64_t)payload[2 * t + 1] << 32; }

enum class ListStatus { Ok, Null, Header };

// bsg_match_pair_rows_list: any tag expanded to the ascending set-relative indices; *out_n the full count, at most cap written.
// Header: a count or an index that the set's rows cannot hold, indices that do not ascend, DENSE bits past the last row.
inline ListStatus pair_rows_list(uint32_t hdr, const uint32_t *payload, uint32_t set_rows, uint32_t *out_rows, uint32_t cap, uint32_t *out_n)
{
    if (!out_n || (cap && !out_rows)) return ListStatus::Null;
    const uint32_t tag = hdr >> 30, n = hdr & 0x3FFFFFFFu, T = tiles_of(set_rows);
    *out_n = 0;
    if (tag == kPairNone || tag == kPairAll) {
        if (n || (tag == kPairAll && set_rows == 0)) return ListStatus::Header;
        if (tag == kPairAll) {
            *out_n = set_rows;
            for (uint32_t i = 0; i < std::min(cap, set_rows); ++i) out_rows[i] = i;
        }
        return ListStatus::Ok;
    }
    if (tag == kPairList ? (n == 0 || n >= set_rows || n >= 2ull * T) : n != 0) return ListStatus::Header;
    if (!payload) return ListStatus::Null;
    if (tag == kPairList) {
        for (uint32_t i = 0; i < n; ++i)
            if (payload[i] >= set_rows || (i && payload[i] <= payload[i - 1])) return ListStatus::Header;
        *out_n = n;
        std::copy(payload, payload + std::min(cap, n), out_rows);
        return ListStatus::Ok;
    }
    uint32_t k = 0;
    for (uint32_t t = 0; t < T; ++t) {
        uint64_t w = dense_word(payload, t);
        if (t + 1 == T && set_rows % 64u && (w >> (set_rows % 64u))) return ListStatus::Header;
        for (; w; w &= w - 1, ++k)
            if (k < cap) out_rows[k] = t * 64u + (uint32_t)__builtin_ctzll(w);
    }
    *out_n = k;
    return ListStatus::Ok;
}

// One device's share of a pair: the part's header over its `rows` rows of the set, which begin at the set's tile `tile0`, and its
// payload (LIST indices are set-relative already: the write pass adds tile0; DENSE words are the part's own tiles).
struct PairPiece {
    uint32_t hdr, rows, tile0;
    const uint32_t *payload;
};

inline uint64_t piece_count(const PairPiece &pc)
{
    const uint32_t tag = pc.hdr >> 30;
    if (tag == kPairNone) return 0;
    if (tag == kPairAll) return pc.rows;
    if (tag == kPairList) return pc.hdr & 0x3FFFFFFFu;
    uint64_t c = 0;
    for (uint32_t t = 0; t < tiles_of(pc.rows); ++t) c += (uint64_t)__builtin_popcountll(dense_word(pc.payload, t));
    return c;
}

// The stitch of a multi-device call: a pair's pieces in row order (a set cut at set-relative multiples of 64 rows has one per
// device) -> the header over the whole set's R rows by the rule above.
inline uint32_t stitch_header(const PairPiece *pieces, uint32_t n, uint32_t R)
{
    uint64_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c += piece_count(pieces[i]);
    return pair_header(c, R);
}
// ... and its canonical payload behind that header (pair_payload_size(hdr, R) u32 at out): LIST = the pieces' indices one after
// the other (ascending, as the pieces are), DENSE = the pieces scattered back into the set's words.
inline void stitch_payload(const PairPiece *pieces, uint32_t n, uint32_t R, uint32_t hdr, uint32_t *out)
{
    const uint32_t tag = hdr >> 30;
    if (tag == kPairList) {
        for (uint32_t i = 0; i < n; ++i) {
            const PairPiece &pc = pieces[i];
            const uint32_t ptag = pc.hdr >> 30;
            if (ptag == kPairAll) {
                for (uint32_t r = 0; r < pc.rows; ++r) *out++ = pc.tile0 * 64u + r;
            } else if (ptag == kPairList) {
                out = std::copy(pc.payload, pc.payload + (pc.hdr & 0x3FFFFFFFu), out);
            } else if (ptag == kPairDense) {
                for (uint32_t t = 0; t < tiles_of(pc.rows); ++t)
                    for (uint64_t w = dense_word(pc.payload, t); w; w &= w - 1) *out++ = (pc.tile0 + t) * 64u + (uint32_t)__builtin_ctzll(w);
            }
        }
    } else if (tag == kPairDense) {
        std::fill(out, out + 2ull * tiles_of(R), 0u);
        for (uint32_t i = 0; i < n; ++i) {
            const PairPiece &pc = pieces[i];
            const uint32_t ptag = pc.hdr >> 30;
            if (ptag == kPairAll) {
                for (uint32_t r = pc.tile0 * 64u; r < pc.tile0 * 64u + pc.rows; ++r) out[r / 32u] |= 1u << (r % 32u);
            } else if (ptag == kPairList) {
                for (uint32_t k = 0; k < (pc.hdr & 0x3FFFFFFFu); ++k) out[pc.payload[k] / 32u] |= 1u << (pc.payload[k] % 32u);
            } else if (ptag == kPairDense) {
                std::copy(pc.payload, pc.payload + 2ull * tiles_of(pc.rows), out + 2ull * pc.tile0);
            }
        }
    }
}

// One part's result as the stitch reads it: its sets, its headers (from its first pair on), its payload and where each pair's begins.
struct PartRows {
    const PartSets *ps;
    const uint32_t *hdr, *payload;
    std::vector<uint64_t> off;             // pair_payload_offsets over ps
};

// The pieces of pair p of set s among the call's parts (in row order), at most parts.size().  A set without rows lies in no part.
inline uint32_t pair_pieces(const std::vector<PartRows> &parts, uint32_t s, uint32_t p, PairPiece *pieces)
{
    uint32_t n = 0;
    for (const PartRows &pr : parts) {
        const PartSets &ps = *pr.ps;
        if (s < ps.s0 || s >= ps.s0 + ps.n()) continue;
        const uint32_t ls = s - ps.s0, lp = p - ps.pair_off[0];
        pieces[n++] = PairPiece{pr.hdr[lp], ps.first_row[ls + 1] - ps.first_row[ls], ps.tile0[ls], pr.payload + pr.off[lp]};
    }
    return n;
}

// The call's headers from its parts' (out_hdr [n_pairs]) and the payload's length ...
inline uint64_t stitch_headers(const std::vector<PartRows> &parts, const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets,
                               uint32_t *out_hdr)
{
    std::vector<PairPiece> pieces(parts.size());
    uint64_t at = 0;
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t R = set_first_row[s + 1] - set_first_row[s];
        for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) {
            out_hdr[p] = stitch_header(pieces.data(), pair_pieces(parts, s, p, pieces.data()), R);
            at += pair_payload_size(out_hdr[p], R);
        }
    }
    return at;
}
// ... and, once the caller's buffer is known to hold it, the payload behind them.
inline void stitch_payloads(const std::vector<PartRows> &parts, const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets,
                            const uint32_t *hdr, uint32_t *out_payload)
{
    std::vector<PairPiece> pieces(parts.size());
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t R = set_first_row[s + 1] - set_first_row[s];
        for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) {
            const uint64_t size = pair_payload_size(hdr[p], R);
            if (size) stitch_payload(pieces.data(), pair_pieces(parts, s, p, pieces.data()), R, hdr[p], out_payload);
            out_payload += size;
        }
    }
}

// What the device's passes read per local set of a part (match.hip.h PairSetDesc): the first of its pairs (counted from the part's
// first), where that pair's words begin in the part's result, the part's rows of the set and the set's tile they begin at.  One
// more entry closes the table: pair0 = the part's pairs.
struct PairSet {
    uint64_t word0;
    uint32_t pair0, rows, tile0, pad;
};
inline std::vector<PairSet> pair_sets(const PartSets &ps)
{
    std::vector<PairSet> v;
    uint64_t at = 0;
    for (uint32_t ls = 0; ls < ps.n(); ++ls) {
        const uint32_t rows = ps.first_row[ls + 1] - ps.first_row[ls];
        v.push_back(PairSet{at, ps.pair_off[ls] - ps.pair_off[0], rows, ps.tile0[ls], 0u});
        at += (uint64_t)tiles_of(rows) * (ps.pair_off[ls + 1] - ps.pair_off[ls]);
    }
    v.push_back(PairSet{at, ps.pair_off[ps.n()] - ps.pair_off[0], 0u, 0u, 0u});
    return v;
}

}  // namespace bsh_wide
