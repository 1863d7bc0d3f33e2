// match.hip.h — the final row test on the device:
//   compileRowMatcher / matchRowBytes / match / matchLeafTokens / evalMatcherNode, row_matcher.go:257-626
// for Field / Token / FieldToken conditions.  The same resumable walker as k_ingest_rows enumerates the row; every
// emission's 256-bit base hash is compared with the conditions' (field and token strings hashed separately:
// FieldToken compares the (path, token) PAIR at one leaf, never the joined "path::token" key — row_matcher.go:587),
// satisfaction flags are monotone, and the expression is evaluated once the walk is over (the reference's early exit
// changes cost, not verdicts).  Equality is decided on all four hash words of an entry AND its keyed 64-bit fingerprint
// (ingest.hip.h, FpKey): an emission whose hashes equal a condition's but whose fingerprint differs is a murmur3 state
// collision — the row is handed to the host matcher, which compares bytes as matchRowBytes does.
// Rows outside the device walker's envelope are reported back and decided by the host matcher too.
//
// FieldRegex conditions (kind 3, k_match_rows_regex = the same body with REGEX = true): each pattern is a byte DFA compiled
// on the host (host/regex_dfa.hpp) whose tables sit in LDS behind the plain matcher's.  At a leaf request the converged part
// of the loop decides which regex conditions see the leaf (its path equals the field or starts with field + ".",
// row_matcher.go hasStringPrefix) by a byte compare of the lane's path buffer; the lane keeps those conditions' DFA states
// in registers (at most kRxActive per leaf, more make the row a fallback row) and the walker feeds them the leaf's
// candidate text (leafTokenInput) one byte at a time, one LDS lookup each.  A condition leaves the active set once it
// accepts (its flag is set) or its DFA is dead; the states still active when the leaf closes are checked for
// accept-at-end.  null is never a candidate text.
//
// A batch of queries in one walk (k_match_rows_many / k_match_rows_many_tok = the same body with MANY = true): the table holds
// the DISTINCT conditions of up to kMatchManyMaxQueries queries, the walk collects the same 64-bit `sat` mask per row, and the
// epilogue evaluates one lowered program per query over it (programs concatenated in LDS behind a prog_off table, at most
// kMatchManyMaxOps ops in all, each of depth <= 64).  Query q's verdicts form bit-plane q of out_bits, laid out as the single
// call's result.  Rows come grouped in sets (one surviving block each) with a u64 query mask per set: a lane looks its set up
// once (binary search in global memory), a verdict is ANDed with its mask bit, a row with mask 0 is never walked (so never a
// fallback row) and a wave of such rows skips the walk altogether.  A row with a non-zero mask that leaves the walker's envelope
// or collides with ANY table condition is a fallback row: all its plane bits are 0.
// LDS of the MANY instance: conditions 5 632 + programs 8 192 + prog_off 260 + lanes 29 696 = 43 780 bytes, three workgroups
// per CU as k_match_rows.
//
// Both together (k_match_rows_many_regex / k_match_rows_many_regex_tok = REGEX and MANY): the table also holds the DISTINCT
// FieldRegex conditions of the batch, their blob sits behind the MANY instance's 43 780 bytes (at most kRxManyLdsCap = 38 140
// bytes of it: 80 KiB in all, 2 workgroups per CU as k_match_rows_regex) and carries, behind its header, one u64 per regex slot:
// the queries whose program references the condition.  A leaf opens a condition's DFA only on a row whose set mask selects one
// of those queries, so a lane's kRxManyActive slots hold what the row's own queries need, and a row is handed back for too many
// regex conditions on one leaf only when the queries live on its set put them there.
//
// Any number of queries (bsg_match_rows_wide): the work is split as the probe side splits it.  k_match_rows_store / _tok / _regex /
// _regex_tok = the same body with WIDE = true: the walk collects `sat` over the table's <= 64 distinct conditions and STORES it per row
// with a state byte (not walked / decided / fallback) instead of evaluating anything; it holds no program in LDS (conditions 5 632 +
// lanes 29 696 = 35 328 bytes, three workgroups per CU; with regex tables of at most kRxWideLdsCap = 46 592 bytes 80 KiB, two).  Rows come
// in sets with a CSR list of the queries evaluated on each: a set with an empty list is never walked, and a leaf opens a regex
// condition's DFA only when the set's condition mask (the OR of the conditions its queries' programs reference) selects it.
// k_eval_row_programs then evaluates the programs over the stored words: a wave owns 64 consecutive rows of ONE set (tiles are
// set-relative) and a range of the set's pairs, loads each lane's sat and state once, reads a pair's query and program on the scalar
// path (constant address space: uniform addresses) and writes __ballot(decided && verdict) as the pair's word of the tile.  No LDS,
// no limit on the number of queries.
//
// The same pairs as tagged row lists (bsg_match_rows_wide_rows): k_pair_sizes, k_pair_scan_sums / _blocks / _apply and k_pair_write
// run behind k_eval_row_programs over the words it left on the device: a header per pair (NONE / ALL / LIST / DENSE by the count of
// its matching rows), an exclusive scan of the payload sizes over any number of pairs, then the LIST indices or the DENSE words
// written back to back.  Headers and payload travel to the host, the words do not.
//
// Substring conditions (kinds 4 and 5, k_match_rows_substr* / k_match_rows_many_substr* = the same body with SUB = true): "some leaf's
// candidate text contains the needle", decided exactly by a third text consumer beside RxNone and RxLaneT.  SubLane runs shift-and
// (bitap) over ALL of the call's needles at once: the host folds the needles as the call's tokenizer folds text and packs them
// first-fit into kSubWords words of 64 bit positions (host/substring_pack.hpp), M[b] has the positions whose needle byte is b, START
// the first position of every needle.  Per folded text byte a lane reads M[b] once from LDS (16 bytes) and steps
// D = ((D << 1) | START) & M[b], hit |= D & active — whatever the number of needles.  A leaf request clears D (no carry between
// leaves) and sets active = ANY, the end positions of the any-field needles (0 for null); the condition loop ORs in the end bit of
// every FieldSubstring condition whose field equals the leaf's path (FieldToken's hash-and-fingerprint compare).  After the walk a
// condition whose end bit is in `hit` is satisfied.  The consumer folds what it is fed as the tokenizer would: ASCII A-Z + 32, a
// rune through the walker's lower table (unknown to the table: a fallback row); without BSG_TOK_LOWER bytes go in as they are.
// LDS: the 4 096-byte table behind the instance's own bytes (the batched instance's 43 780 rounded up to 16: M[b] is one 16-byte read).
//
// Both text consumers in one walk (k_match_rows_regex_substr* / k_match_rows_many_regex_substr* = REGEX and SUB): every candidate text
// byte goes to the RxLaneT (raw) and to the SubLane (folded), a leaf request runs both parents' handling, and a row is a fallback row
// by either parent's rule.  LDS: the needle table where the substring instances have it, the regex blob behind the table (at most
// kRxSubLdsCap = 40 448 / kRxManySubLdsCap = 34 032 bytes: 80 KiB in all, two workgroups per CU as the regex walkers).
//
// Substring conditions in the storing walker (bsg_match_rows_wide_substr, k_match_rows_store_substr* / k_match_rows_store_regex_substr* =
// WIDE and SUB): the needle table sits at kMatchWideLdsBytes = 35 328 (a multiple of 16), 39 424 bytes in all and three workgroups per CU;
// with regex tables (at most kRxWideSubLdsCap = 42 496 bytes) 80 KiB, two.  Regex conditions stay gated by the set's condition mask,
// needles are not: every needle of the table listens on every walked row, and the flag of a condition none of the set's queries
// references is unspecified (nothing reads it).  A row is a fallback row by the union of the parents' rules.
//
// Numeric range conditions (kind 6, k_match_rows_range* / k_match_rows_many_range* = the same body with RANGE = true): "some number leaf
// whose path EQUALS the field has a value inside [lo, hi]" (int64 bounds, each closed, open or absent), decided exactly by a fourth text
// consumer.  NumLane parses the raw literal the walker feeds byte by byte into sign, a u64 magnitude of the integer digits with a sticky
// overflow bit, and "the fraction has a non-zero digit": one parse per leaf, a few registers, nothing in LDS.  A leaf request decides the
// number still pending against every range condition listening on ITS leaf (leaf_mask, FieldToken's hash-and-fingerprint compare of the
// path), then the condition loop marks the conditions listening on the new leaf; the last number is decided after the walk.  The
// compare is integer arithmetic on (sign, magnitude, overflow, fraction): there is no float64 round trip.  A literal with an exponent on
// a leaf ANY range condition of the table listens on makes the row a fallback row (the host compares digit strings).  The bounds sit in
// the condition's record where a token's hash words would (e[4] = lo, e[5] = hi), the flags in bits 8-11 of e[10]: no byte of LDS is added.
//
// Range conditions in the storing walker (bsg_match_rows_wide_range, k_match_rows_store_range* = WIDE and RANGE): kMatchWideLdsBytes and three
// workgroups per CU as k_match_rows_store.  A range condition listens on a leaf only where the row's set lists a query that uses it
// (the set's condition mask, the gate of the regex header loop), so an exponent literal hands a row back only if such a condition sits
// on its leaf; the batched walker asks ANY condition of the table.  The flag of a range condition none of the set's queries references
// is unspecified (nothing reads it).
//
// Range conditions beside the text consumers (kinds 0-6, k_match_rows_regex_substr_range* / k_match_rows_many_regex_substr_range* = REGEX, SUB
// and RANGE): RxSubNumFeed hands every byte of a number literal to the DFAs, the needles and NumLane, a string's bytes to the first two.
// Every statement the three flags guard runs as in the parents; a row is a fallback row by the union of their rules.  In the batched
// instances a DFA opens only for a row whose set mask selects a user of the condition, needles are ungated, and an exponent literal on
// the field of ANY range condition of the table hands the row back.  No LDS beyond the regex_substr instances', two workgroups per CU.
//
// All three in the storing walker (bsg_match_rows_wide_regex_substr_range, k_match_rows_store_regex_substr_range* = WIDE, REGEX, SUB and
// RANGE): the union of the wide parents.  A DFA opens, and a range condition listens, only where the set's condition mask selects the
// condition; every needle listens on every walked row; the flag of a condition none of the set's queries references is unspecified
// (nothing reads it).  So an exponent literal hands a row back only if a range condition of the SET's queries sits on its leaf, and five
// regex conditions on one leaf only if the set's queries put them there - not the batched walker's "any condition of the table".  One
// family serves every mix beside a range condition: the needle table always sits at kMatchWideLdsBytes (all zero without a needle), the
// blob behind it (n_rx = n_words = 0 without a regex condition), at most kRxWideSubLdsCap = 42 496 bytes needle or not: 80 KiB and two
// workgroups per CU with a blob at the cap, 39 424 bytes and three without one.
#pragma once
#include <type_traits>
#include "ingest.hip.h"
#include "host/row_program.hpp"

namespace bsg {

constexpr uint32_t kMatchMaxConds = 64;    // satisfaction flags live in one u64 per row
constexpr uint32_t kMatchMaxOps = 512;
constexpr uint32_t kMatchCondWords = 11;   // hf[4], ht[4], fingerprint of the field string, of the token string, kind

struct MatchArgs {
    const uint8_t *rows;
    const uint64_t *row_off;
    const uint64_t *cond_h;      // [2 * n_conds][4]: base hashes of condition c's field string (2c) and token string (2c + 1)
    const uint64_t *cond_fp;     // [2 * n_conds]: their keyed fingerprints
    const uint32_t *cond_kind;   // [n_conds]
    const uint32_t *prog;        // lowered postfix program: TERM i / AND2 / OR2 / TRUE / FALSE (opcodes 0,1,2,3,4)
    const uint32_t *lower;
    uint64_t *out_bits;          // bit r & 63 of word r >> 6: row r matches
    uint32_t *fallback_rows;
    uint32_t *n_fallback;
    uint32_t n_rows, n_conds, n_ops;
    uint32_t row_base;           // added to the row indices reported in fallback_rows (a launch covers rows [row_base, row_base + n_rows) of the call;
                                 // row_off / out_bits already point at its first row / word)
    FpKey key;
};

constexpr uint32_t kMatchLdsBytes = kMatchMaxConds * kMatchCondWords * 8 + kMatchMaxOps * 4 + kIngestThreads * kLaneLds;

// ---- a batch of queries over one condition table (k_match_rows_many) ----
constexpr uint32_t kMatchManyMaxQueries = 64;   // one mask bit per query and set
constexpr uint32_t kMatchManyMaxOps = 2048;     // lowered ops of all programs together: 8 KiB of LDS
constexpr uint32_t kMatchManyProgBytes = kMatchManyMaxOps * 4 + (kMatchManyMaxQueries + 1) * 4;   // programs, then prog_off
constexpr uint32_t kMatchManyLdsBytes = kMatchMaxConds * kMatchCondWords * 8 + kMatchManyProgBytes + kIngestThreads * kLaneLds;
static_assert(3u * kMatchManyLdsBytes <= 160u * 1024u, "k_match_rows_many keeps three workgroups per CU");
// MatchArgs::prog holds the concatenated lowered programs (n_ops = their total), out_bits plane 0
struct MatchManyArgs {
    const uint32_t *prog_off;        // [n_queries + 1] into MatchArgs::prog
    const uint32_t *set_first_row;   // [n_sets + 1], in the rows MatchArgs::row_base counts; first 0, last = their number
    const uint64_t *set_mask;        // [n_sets]: bit q = evaluate query q on this set's rows
    uint64_t plane_words;            // words between two planes of out_bits
    uint32_t n_queries, n_sets;      // n_sets == 0: every query on every row
};

// ---- FieldRegex conditions ----
constexpr uint32_t kRxMaxConds = 16;       // regex conditions per call
constexpr uint32_t kRxActive = 4;          // regex conditions one leaf may feed at once (registers per lane)
constexpr uint32_t kRxLdsCap = 80u * 1024u - kMatchLdsBytes;   // table bytes: the regex kernel keeps 2 workgroups per CU
#ifndef BSG_RX_MANY_SLOTS                   // a lab build may try another slot count (tools/regex_many_lab.py); the library ships 4
#define BSG_RX_MANY_SLOTS 4
#endif
constexpr uint32_t kRxManyActive = BSG_RX_MANY_SLOTS;          // the same per leaf in the batched regex kernels (4 against 8: DESIGN.md section 9)
constexpr uint32_t kRxManyLdsCap = 80u * 1024u - kMatchManyLdsBytes;   // their table bytes, user masks included
static_assert(kRxManyLdsCap == 38140u && 2u * (kMatchManyLdsBytes + kRxManyLdsCap) <= 160u * 1024u,
              "k_match_rows_many_regex keeps two workgroups per CU");
// LDS table blob, built by the host (host/regex_groups.hpp build_blob):
//   header [n_rx][4] u32: { region offset | (n_classes - 1) << 16 | slot << 24,  start entry | condition index << 16,
//                           field offset | field length << 16,  0 }
//   per pattern (4-byte aligned region): class map [256] u8, then transitions [n_states * n_classes] u16 whose entries are
//   target state | kRxAccept / kRxDead / kRxAcceptAtEnd of the target; then the field strings.
//   The batched call's blob holds, between the header and the first region, users [n_rx] u64: bit q = query q's program
//   references the condition (host/regex_groups.hpp user_masks).
constexpr uint32_t kRxAccept = 0x8000u, kRxDead = 0x4000u, kRxAcceptAtEnd = 0x2000u, kRxStateMask = 0x1FFFu;
struct RxArgs {
    const uint32_t *blob;       // the table blob as words
    uint32_t n_words, n_rx;
};
// ---- any number of queries: the walk stores, k_eval_row_programs evaluates (bsg_match_rows_wide) ----
constexpr uint32_t kMatchWideLdsBytes = kMatchMaxConds * kMatchCondWords * 8 + kIngestThreads * kLaneLds;   // no programs in LDS
static_assert(3u * kMatchWideLdsBytes <= 160u * 1024u, "k_match_rows_store keeps three workgroups per CU");
constexpr uint32_t kRxWideLdsCap = 80u * 1024u - kMatchWideLdsBytes;   // regex table bytes of the storing walker (no user masks in its blob)
static_assert(kRxWideLdsCap == 46592u && kRxWideLdsCap <= 0x10000u && 2u * (kMatchWideLdsBytes + kRxWideLdsCap) <= 160u * 1024u,
              "k_match_rows_store_regex keeps two workgroups per CU, and the blob's 16-bit offsets reach all of it");
constexpr uint8_t kRowNotWalked = 0, kRowDecided = 1, kRowFallback = 2;
struct MatchWideArgs {
    const uint32_t *set_first_row;   // [n_sets + 1], in the rows MatchArgs::row_base counts; n_sets >= 1 (the host makes the implicit set)
    const uint64_t *set_cond_mask;   // [n_sets]: bit c = a program of a query listed on the set references condition c
    const uint32_t *set_pair_off;    // [n_sets + 1]: the set's pairs; an empty range = the set's rows are not walked
    uint64_t *sat;                   // [n_rows] of the launch: the row's satisfaction flags
    uint8_t *state;                  // [n_rows] of the launch: kRowNotWalked / kRowDecided / kRowFallback
    uint32_t n_sets;
};
// one wave of k_eval_row_programs (host/wide_plan.hpp RowEvalItem, read as four u64 on the scalar path)
struct RowEvalItem {
    uint64_t out0;
    uint32_t row0, n_rows, pair0, pair1, stride, pad;
};
struct RowEvalArgs {
    const RowEvalItem *items;
    const uint32_t *pairs;           // the part's pairs: the query of each
    const uint32_t *prog_off;        // [n_queries + 1] into prog
    const uint32_t *prog;            // the lowered programs
    const uint64_t *sat;
    const uint8_t *state;
    uint64_t *out;                   // the part's result words
    uint32_t n_items;
};
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// one lane's active regex conditions (hd = header word 0 of the condition, ~0u = free slot; st = its DFA entry)
template <uint32_t SLOTS>
struct RxLaneT {
    const lds_u8 *tab;
    uint32_t hd[SLOTS], st[SLOTS];
    uint32_t sat;                                   // bit j: regex slot j matched a candidate text of this row
    __device__ __forceinline__ void feed(uint32_t b)
    {
#pragma unroll
        for (uint32_t k = 0; k < SLOTS; ++k)
            if (hd[k] != ~0u) {
                const uint32_t off = hd[k] & 0xFFFFu, ncls = ((hd[k] >> 16) & 0xFFu) + 1u;
                const uint32_t v = ((const lds_u16 *)(tab + off + 256u))[(st[k] & kRxStateMask) * ncls + tab[off + b]];
                st[k] = v;
                if (v & (kRxAccept | kRxDead)) {
                    if (v & kRxAccept) sat |= 1u << (hd[k] >> 24);
                    hd[k] = ~0u;
                }
            }
    }
    __device__ __forceinline__ void feed_run(uint64_t v, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i) feed(c_at(v, i));
    }
    __device__ __forceinline__ void feed_rune(uint32_t r)
    {
        uint32_t n = 1;
        const uint32_t bytes = rune_utf8(r, n);
        for (uint32_t i = 0; i < n; ++i) feed((bytes >> (8u * i)) & 0xFFu);
    }
    __device__ __forceinline__ void close()
    {
#pragma unroll
        for (uint32_t k = 0; k < SLOTS; ++k) {
            if (hd[k] != ~0u && (st[k] & kRxAcceptAtEnd)) sat |= 1u << (hd[k] >> 24);
            hd[k] = ~0u;
        }
    }
};

typedef RxLaneT<kRxActive> RxLane;

// ---- substring conditions ----
constexpr uint32_t kSubWords = 2;                                  // 64 needle bytes each
constexpr uint32_t kSubTableBytes = 256u * kSubWords * 8u;         // M[256][kSubWords]
constexpr uint32_t kMatchSubLdsBytes = kMatchLdsBytes + kSubTableBytes;
constexpr uint32_t kMatchManySubBase = (kMatchManyLdsBytes + 15u) & ~15u;
constexpr uint32_t kMatchManySubLdsBytes = kMatchManySubBase + kSubTableBytes;
static_assert(kSubWords == 2u && kMatchLdsBytes % 16u == 0u && kMatchSubLdsBytes == 37376u + 4096u && kMatchManySubLdsBytes == 43780u + 12u + 4096u &&
                  3u * kMatchSubLdsBytes <= 160u * 1024u && 3u * kMatchManySubLdsBytes <= 160u * 1024u,
              "k_match_rows_substr and k_match_rows_many_substr keep three workgroups per CU, their tables 16-byte aligned");
struct SubArgs {
    const uint64_t *table;                  // M[256][kSubWords]
    uint64_t start[kSubWords], any[kSubWords];
};
// A condition's LDS record e[10] in these kernels: kind | word of its needle << 8 | end bit << 16 (kinds 4 and 5; else the kind alone).
// One lane's shift-and state over the call's packed needles.
struct SubLane {
    const lds_u64i *m;
    const Walker *wk;                       // its lower table, and whether the current leaf is one that is never emitted
    uint64_t s0, s1, d0, d1, a0, a1, h0, h1;
    bool lower, fail;
    __device__ __forceinline__ void step(uint32_t b)
    {
        const lds_u64i *e = m + b * kSubWords;
        const uint64_t m0 = e[0], m1 = e[1];
        d0 = ((d0 << 1) | s0) & m0;
        d1 = ((d1 << 1) | s1) & m1;
        if (!wk->quiet) { h0 |= d0 & a0; h1 |= d1 & a1; }          // a leaf without a path has no request: it is no candidate text
    }
    __device__ __forceinline__ void feed(uint32_t b)
    {
        if (lower && b - (uint32_t)'A' < 26u) b += 32u;
        step(b);
    }
    __device__ __forceinline__ void feed_run(uint64_t v, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i) feed(c_at(v, i));
    }
    __device__ __forceinline__ void feed_rune(uint32_t r)          // r >= 0x80
    {
        if (lower) {
            const uint32_t lo = r < 0x20000u ? wk->lower[r] : 0u;
            if (lo == 0xFFFFFFFFu) { fail = true; return; }
            if (lo != 0u) r = lo;
        }
        if (r < 0x80u) { step(r); return; }                        // U+212A -> 'k': lower case already
        uint32_t n = 1;
        const uint32_t bytes = rune_utf8(r, n);
        for (uint32_t i = 0; i < n; ++i) step((bytes >> (8u * i)) & 0xFFu);
    }
};

// FieldRegex and substring conditions in one walk (k_match_rows_regex_substr* / k_match_rows_many_regex_substr*): the text consumer is
// both lanes at once.  The DFAs step over the raw bytes, the needles over the folded ones.  The two lanes stay two objects and this
// one only refers to them: SubLane::wk points at the Walker, and a lane object that held that pointer BESIDE RxLaneT's hd[] / st[]
// (indexed by loops that are unrolled late) stays in private memory past the first scalar replacement, the Walker with it; by the
// next one hs_absorb's `if (t < 8) s.lo |= v; else s.hi |= v;` on the in-memory w.tok has become one access at a computed offset
// and the Walker can no longer be split: 304 bytes of scratch per lane in the default and the separator instances.
template <uint32_t SLOTS>
struct RxSubFeed {
    RxLaneT<SLOTS> &rx;
    SubLane &sub;
    __device__ __forceinline__ void feed(uint32_t b) { rx.feed(b); sub.feed(b); }
    __device__ __forceinline__ void feed_run(uint64_t v, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i) feed(c_at(v, i));
    }
    __device__ __forceinline__ void feed_rune(uint32_t r) { rx.feed_rune(r); sub.feed_rune(r); }
};
// LDS of the two instances: the needle table where the substring instances have it, the regex blob behind the table
constexpr uint32_t kRxSubLdsCap = 80u * 1024u - kMatchSubLdsBytes;
constexpr uint32_t kRxManySubLdsCap = 80u * 1024u - kMatchManySubLdsBytes;
// ... and of the storing walker's two (k_match_rows_store_substr* / k_match_rows_store_regex_substr*): the table behind the lanes, then the blob
constexpr uint32_t kMatchWideSubLdsBytes = kMatchWideLdsBytes + kSubTableBytes;
constexpr uint32_t kRxWideSubLdsCap = 80u * 1024u - kMatchWideSubLdsBytes;
static_assert(kMatchWideLdsBytes % 16u == 0u && kMatchWideSubLdsBytes == 35328u + 4096u && 3u * kMatchWideSubLdsBytes <= 160u * 1024u &&
                  kRxWideSubLdsCap == 42496u && kRxWideSubLdsCap <= 0x10000u && 2u * (kMatchWideSubLdsBytes + kRxWideSubLdsCap) <= 160u * 1024u,
              "k_match_rows_store_substr keeps three workgroups per CU, its table 16-byte aligned; k_match_rows_store_regex_substr two, and the blob's 16-bit offsets reach all of it");
static_assert(kRxSubLdsCap == 40448u && kRxManySubLdsCap == 34032u && kRxSubLdsCap <= 0x10000u && kMatchSubLdsBytes % 4u == 0u && kMatchManySubLdsBytes % 4u == 0u &&
                  2u * (kMatchSubLdsBytes + kRxSubLdsCap) <= 160u * 1024u && 2u * (kMatchManySubLdsBytes + kRxManySubLdsCap) <= 160u * 1024u,
              "k_match_rows_regex_substr and k_match_rows_many_regex_substr keep two workgroups per CU, and the blob's 16-bit offsets reach all of it");

// ---- numeric range conditions ----
// A condition's LDS record e[10] in these kernels: kind | flags << 8 (kind 6; else the kind alone); e[4] = lo, e[5] = hi as two's complement.
constexpr uint32_t kRangeNoLo = 1u, kRangeNoHi = 2u, kRangeLoOpen = 4u, kRangeHiOpen = 8u;   // bloomgpu.h BSG_RANGE_*
// The range walkers add no LDS: each keeps its RANGE-less sibling's bytes, and so its three workgroups per CU.
static_assert(3u * kMatchLdsBytes <= 160u * 1024u && 3u * kMatchManyLdsBytes <= 160u * 1024u,
              "k_match_rows_range and k_match_rows_many_range keep three workgroups per CU as k_match_rows and k_match_rows_many");
static_assert(3u * kMatchWideLdsBytes <= 160u * 1024u, "k_match_rows_store_range keeps three workgroups per CU as k_match_rows_store");
// One lane's number parser: the raw literal of the current number leaf as -?digits[.digits][(e|E)...], fed byte by byte.
struct NumLane {
    const Walker *wk;                       // whether the current leaf is one that is never emitted
    uint64_t mag;                           // the integer digits' value mod 2^64 ...
    bool on;                                // the current leaf is a number some range condition listens on
    bool neg, ovf, point, frac, expo;        // '-' seen; ... and whether it passed 2^64 - 1; '.' seen; a non-zero fraction digit; an exponent part
    __device__ __forceinline__ void open(bool listen)
    {
        on = listen; mag = 0; neg = ovf = point = frac = expo = false;
    }
    __device__ __forceinline__ void feed(uint32_t b)
    {
        if (!on || wk->quiet || expo) return;                       // a leaf without a path has no request: its bytes belong to no number of ours
        const uint32_t d = b - (uint32_t)'0';
        if (d <= 9u) {
            if (point) frac |= d != 0u;
            else {
                ovf |= mag > 1844674407370955161ULL || (mag == 1844674407370955161ULL && d > 5u);   // mag * 10 + d > 2^64 - 1
                mag = mag * 10u + d;
            }
        }
        else if (b == '-') neg = true;
        else if (b == '.') point = true;
        else expo = true;                                           // 'e' / 'E': the host decides this literal
    }
    __device__ __forceinline__ void feed_run(uint64_t, uint32_t) {}   // only strings reach these two
    __device__ __forceinline__ void feed_rune(uint32_t) {}
    // |value| = mag + f, 0 <= f < 1, f != 0 iff frac; against a magnitude k
    __device__ __forceinline__ bool mag_ge(uint64_t k) const { return ovf || mag >= k; }
    __device__ __forceinline__ bool mag_gt(uint64_t k) const { return ovf || mag > k || (mag == k && frac); }
    // the parsed value inside the interval (lo, hi as two's complement, flags kRange*)
    __device__ __forceinline__ bool inside(uint64_t lo, uint64_t hi, uint32_t flags) const
    {
        const bool below = neg && (mag != 0ull || frac || ovf);    // -0 and -0.0 are 0
        const bool lo_neg = (int64_t)lo < 0, hi_neg = (int64_t)hi < 0;
        const uint64_t alo = lo_neg ? 0ull - lo : lo, ahi = hi_neg ? 0ull - hi : hi;   // |INT64_MIN| = 2^63 fits
        bool lo_ok, hi_ok;
        if (!below) {                                              // value >= 0
            lo_ok = lo_neg || ((flags & kRangeLoOpen) ? mag_gt(alo) : mag_ge(alo));
            hi_ok = !hi_neg && ((flags & kRangeHiOpen) ? !mag_ge(ahi) : !mag_gt(ahi));
        } else {                                                   // value = -(mag + f) < 0: a fraction puts it BELOW its truncated integer part
            lo_ok = lo_neg && ((flags & kRangeLoOpen) ? !mag_ge(alo) : !mag_gt(alo));
            hi_ok = !hi_neg || ((flags & kRangeHiOpen) ? mag_gt(ahi) : mag_ge(ahi));
        }
        return ((flags & kRangeNoLo) || lo_ok) && ((flags & kRangeNoHi) || hi_ok);
    }
};

// All three consumers in one walk (k_match_rows_regex_substr_range* / k_match_rows_many_regex_substr_range*): as RxSubFeed, this one only
// refers to the lanes (it neither derives from them nor holds one by value: the 304 bytes of scratch above).  A number literal arrives
// byte by byte through feed() and is candidate text of the DFAs and the needles AND the digits NumLane parses; runs and runes come from
// strings only, which no range condition reads.
template <uint32_t SLOTS>
struct RxSubNumFeed {
    RxLaneT<SLOTS> &rx;
    SubLane &sub;
    NumLane &num;
    // A leaf without a path raises no request, so nothing closes the DFAs the leaf before it left open: they must not read its bytes
    // (SubLane and NumLane look at Walker::quiet themselves).
    __device__ __forceinline__ void feed(uint32_t b)
    {
        if (!num.wk->quiet) rx.feed(b);
        sub.feed(b);
        num.feed(b);
    }
    __device__ __forceinline__ void feed_run(uint64_t v, uint32_t n)
    {
        const bool heard = !num.wk->quiet;
        for (uint32_t i = 0; i < n; ++i) { const uint32_t b = c_at(v, i); if (heard) rx.feed(b); sub.feed(b); }
    }
    __device__ __forceinline__ void feed_rune(uint32_t r)
    {
        if (!num.wk->quiet) rx.feed_rune(r);
        sub.feed_rune(r);
    }
};

// The number parsed on the leaf that just ended (pending: this lane has one), against every range condition that listened on it.
__device__ __forceinline__ void decide_number(const NumLane &nl, bool pending, const lds_u64i *conds, uint32_t n_conds, uint64_t leaf_mask, uint64_t &sat,
                                              bool &num_fail)
{
    if (__ballot(pending) == 0ull) return;
    if (pending && nl.expo) num_fail = true;
    for (uint32_t c = 0; c < n_conds; ++c) {                             // uniform loop: bounds and flags are LDS broadcasts
        const lds_u64i *e = conds + c * kMatchCondWords;
        const uint32_t rec = (uint32_t)e[10];
        if ((rec & 0xFFu) != 6u) continue;
        if (pending && !nl.expo && ((leaf_mask >> c) & 1ULL) && nl.inside(e[4], e[5], rec >> 8)) sat |= 1ULL << c;
    }
}

// the set of row g: the first s whose rows end behind it (set_first_row[n_sets] = the number of rows > g)
__device__ __forceinline__ uint32_t row_set_of(const uint32_t *set_first_row, uint32_t n_sets, uint32_t g)
{
    uint32_t lo = 0, hi = n_sets - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (set_first_row[mid + 1] <= g) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

template <bool REGEX, class TOK, bool MANY = false, uint32_t SLOTS = kRxActive, bool WIDE = false, bool SUB = false, bool RANGE = false>
__device__ __forceinline__ void match_rows_body(const MatchArgs &a, const RxArgs &x, const TOK &tk, const MatchManyArgs &m = MatchManyArgs{},
                                                const MatchWideArgs &wd = MatchWideArgs{}, const SubArgs &sb = SubArgs{})
{
    static_assert(!(MANY && WIDE), "the storing walker evaluates no program");
    if constexpr (!(REGEX && SUB)) {   // both text consumers: the number consumer may join them, in every walker; never beside exactly one of the two
        static_assert(!(RANGE && (REGEX || SUB)), "range conditions: beside no text consumer, or beside both");
    }
    constexpr uint32_t kSubBase = WIDE ? kMatchWideLdsBytes : MANY ? kMatchManySubBase : kMatchLdsBytes;   // the needle table sits behind the instance's own LDS
    constexpr uint32_t kProgBytes = WIDE ? 0u : MANY ? kMatchManyProgBytes : kMatchMaxOps * 4;
    constexpr uint32_t kRxBase = SUB ? kSubBase + kSubTableBytes : WIDE ? kMatchWideLdsBytes : MANY ? kMatchManyLdsBytes : kMatchLdsBytes;   // the regex blob sits behind the instance's own LDS (and the needle table)
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    lds_u64i *conds = (lds_u64i *)lds_raw;
    typedef __attribute__((address_space(3))) uint32_t lds_u32i;
    lds_u32i *prog = (lds_u32i *)(lds_raw + kMatchMaxConds * kMatchCondWords * 8);
    for (uint32_t c = threadIdx.x; c < a.n_conds; c += kIngestThreads) {
        lds_u64i *e = conds + c * kMatchCondWords;
        for (uint32_t j = 0; j < 4; ++j) { e[j] = a.cond_h[(uint64_t)(2 * c) * 4 + j]; e[4 + j] = a.cond_h[(uint64_t)(2 * c + 1) * 4 + j]; }
        e[8] = a.cond_fp[2 * c]; e[9] = a.cond_fp[2 * c + 1];
        e[10] = a.cond_kind[c];
    }
    if constexpr (!WIDE)
        for (uint32_t i = threadIdx.x; i < a.n_ops; i += kIngestThreads) prog[i] = a.prog[i];
    if constexpr (MANY)
        for (uint32_t i = threadIdx.x; i <= m.n_queries; i += kIngestThreads) prog[kMatchManyMaxOps + i] = m.prog_off[i];
    if constexpr (REGEX)
        for (uint32_t i = threadIdx.x; i < x.n_words; i += kIngestThreads) ((lds_u32 *)(lds_raw + kRxBase))[i] = x.blob[i];
    if constexpr (SUB)
        for (uint32_t i = threadIdx.x; i < 256u * kSubWords; i += kIngestThreads) ((lds_u64i *)(lds_raw + kSubBase))[i] = sb.table[i];
    __syncthreads();
    const uint32_t r = blockIdx.x * kIngestThreads + threadIdx.x;
    const bool live = r < a.n_rows;
    Walker w;
    ChunkCursor cc;
    walker_bind(w, cc, a.rows, (lds_u8 *)lds_raw + kMatchMaxConds * kMatchCondWords * 8 + kProgBytes + threadIdx.x * kLaneLds, a.lower, a.key, false);
    uint64_t qmask = ~0ull;      // MANY: the queries evaluated on this lane's row
    if constexpr (MANY) {
        if (live && m.n_sets) qmask = m.set_mask[row_set_of(m.set_first_row, m.n_sets, a.row_base + r)];
    }
    uint64_t cmask = 0;          // WIDE: the conditions the row's set evaluates; listed: the set has a pair at all
    bool listed = false;
    if constexpr (WIDE) {
        if (live) {
            const uint32_t lo = row_set_of(wd.set_first_row, wd.n_sets, a.row_base + r);
            cmask = wd.set_cond_mask[lo];
            listed = wd.set_pair_off[lo + 1] != wd.set_pair_off[lo];
        }
    }
    const bool walk = WIDE ? listed : MANY ? (live && qmask != 0ull) : live;
    walker_reset(w, cc, walk ? a.row_off[r] : 0, walk ? a.row_off[r + 1] : 0, walk);
    uint32_t res = walk ? R_CONTINUE : R_DONE;
    uint64_t sat = 0, leaf_mask = 0;
    bool collided = false;       // equal hashes, different fingerprint: only the host's byte compare can decide this row
    typename std::conditional<REGEX, RxLaneT<SLOTS>, RxNone>::type rx;   // the text consumers: the regex lane, the substring lane, or both
    typename std::conditional<SUB, SubLane, RxNone>::type sl;
    typename std::conditional<RANGE, NumLane, RxNone>::type nl;
    bool num_fail = false;       // RANGE: an exponent literal on a leaf a range condition listens on: the host decides this row
    bool rx_over = false;        // more regex conditions on one leaf than a lane holds: the host decides this row
    if constexpr (REGEX) {
        rx.tab = (const lds_u8 *)lds_raw + kRxBase;
        rx.sat = 0;
#pragma unroll
        for (uint32_t k = 0; k < SLOTS; ++k) rx.hd[k] = ~0u;
    }
    if constexpr (SUB) {
        sl.m = (const lds_u64i *)(lds_raw + kSubBase);
        sl.wk = &w;
        sl.s0 = sb.start[0]; sl.s1 = sb.start[1];
        sl.d0 = sl.d1 = sl.a0 = sl.a1 = sl.h0 = sl.h1 = 0;
        sl.lower = tk.lower();
        sl.fail = false;
    }
    if constexpr (RANGE) {
        nl.wk = &w;
        nl.open(false);
    }
    while (__ballot(res == R_CONTINUE || w.req != Q_NONE) != 0ull) {
        while (__ballot(res == R_CONTINUE && w.req == Q_NONE) != 0ull)
            if (res == R_CONTINUE && w.req == Q_NONE) {
                if constexpr (REGEX && SUB && RANGE) { RxSubNumFeed<SLOTS> all{rx, sl, nl}; res = advance<true>(w, cc, all, tk); }
                else if constexpr (REGEX && SUB) { RxSubFeed<SLOTS> both{rx, sl}; res = advance<true>(w, cc, both, tk); }
                else if constexpr (SUB) res = advance<true>(w, cc, sl, tk);
                else if constexpr (RANGE) res = advance<true>(w, cc, nl, tk);
                else res = advance<true>(w, cc, rx, tk);
            }
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
        if constexpr (RANGE) decide_number(nl, q == Q_LEAF && nl.on, conds, a.n_conds, leaf_mask, sat, num_fail);   // before leaf_mask forgets who listened
        if (q == Q_LEAF) leaf_mask = 0;
        bool num_listen = false;                                         // RANGE: a range condition listens on this request's leaf
        if constexpr (REGEX) {
            if (q == Q_LEAF) rx.close();                                 // the previous leaf's text ended before this request
            const bool text = q == Q_LEAF && !(w.st == S_LIT && w.lit == 2u);   // null is never a candidate text
            const lds_u32 *hdr = (const lds_u32 *)rx.tab;
            // only a leaf request opens DFAs: the (more frequent) word and field rounds skip the header loop as a whole wave
            for (uint32_t j = 0; j < x.n_rx && __ballot(text) != 0ull; ++j) {   // uniform loop: header words are LDS broadcasts
                const uint32_t h0 = hdr[4 * j], h1 = hdr[4 * j + 1], h2 = hdr[4 * j + 2], flen = h2 >> 16;
                const lds_u8 *fld = rx.tab + (h2 & 0xFFFFu);
                bool under = text && !((rx.sat >> j) & 1u) && flen != 0u && flen <= kPathCap &&
                             (plen == flen || (plen > flen && w.path[flen] == '.'));
                if constexpr (MANY) {                                    // only for a row whose set evaluates a query that uses the condition
                    const uint64_t users = (uint64_t)hdr[4 * x.n_rx + 2 * j] | ((uint64_t)hdr[4 * x.n_rx + 2 * j + 1] << 32);
                    under = under && (qmask & users) != 0ull;
                }
                if constexpr (WIDE) under = under && ((cmask >> (h1 >> 16)) & 1ull) != 0ull;   // ... whose set lists a query that uses it
                for (uint32_t i = 0; i < flen && __ballot(under) != 0ull; ++i)   // ends once no lane's path can still match
                    if (under) under = w.path[i] == fld[i];
                if (under) {
                    const uint32_t sv = h1 & 0xFFFFu;
                    if (sv & kRxAccept) rx.sat |= 1u << j;               // the pattern matches every text (an empty match)
                    else if (!(sv & kRxDead)) {
                        bool placed = false;
#pragma unroll
                        for (uint32_t k = 0; k < SLOTS; ++k)
                            if (!placed && rx.hd[k] == ~0u) { rx.hd[k] = h0; rx.st[k] = sv; placed = true; }
                        rx_over |= !placed;
                    }
                }
            }
        }
        const bool is_path = q == Q_FIELD || q == Q_LEAF, is_word = q == Q_WORD;
        bool sub_text = false;                                           // SUB: this request opens a leaf with a candidate text
        if constexpr (SUB) {
            if (q == Q_LEAF) {                                           // a new leaf: no carry from the one before, the any-field needles listen
                sub_text = !(w.st == S_LIT && w.lit == 2u);              // null is never a candidate text
                sl.d0 = sl.d1 = 0;
                sl.a0 = sub_text ? sb.any[0] : 0ull;
                sl.a1 = sub_text ? sb.any[1] : 0ull;
            }
        }
        for (uint32_t c = 0; c < a.n_conds; ++c) {                       // uniform loop: the conditions come from LDS broadcasts
            const lds_u64i *e = conds + c * kMatchCondWords;
            const uint32_t kind = (SUB || RANGE) ? ((uint32_t)e[10] & 0xFFu) : (uint32_t)e[10];   // 0 Field, 1 Token, 2 FieldToken
            if (REGEX && kind == 3u) continue;                           // FieldRegex: the DFAs above
            if constexpr (RANGE) {
                if (kind == 6u) {                                        // FieldRange: marked like FieldToken, decided by NumLane; e[4], e[5] hold bounds, no token
                    const bool heq = q == Q_LEAF && e[0] == h[0] && e[1] == h[1] && e[2] == h[2] && e[3] == h[3];
                    const bool eq = heq && e[8] == fp;
                    collided |= heq && !eq;
                    bool hears = eq;
                    if constexpr (WIDE) hears = eq && ((cmask >> c) & 1ull) != 0ull;   // ... only where the row's set lists a query that uses it
                    if (hears) { leaf_mask |= 1ULL << c; num_listen = true; }
                    continue;
                }
            }
            if constexpr (SUB) {
                if (kind >= 4u) {                                        // Substring: SubLane decides; FieldSubstring: on the leaves of its own path
                    if (kind == 5u) {
                        const bool heq = is_path && e[0] == h[0] && e[1] == h[1] && e[2] == h[2] && e[3] == h[3];
                        const bool eq = heq && e[8] == fp;
                        collided |= heq && !eq;
                        const uint32_t rec = (uint32_t)e[10];
                        const uint64_t end = 1ULL << ((rec >> 16) & 63u);
                        if (eq && sub_text) { if ((rec >> 8) & 1u) sl.a1 |= end; else sl.a0 |= end; }
                    }
                    continue;
                }
            }
            const uint64_t bit = 1ULL << c;
            if (kind != 1u) {                                            // conditions with a field: compare paths
                const bool heq = is_path && e[0] == h[0] && e[1] == h[1] && e[2] == h[2] && e[3] == h[3];
                const bool eq = heq && e[8] == fp;
                collided |= heq && !eq;
                if (eq && kind == 0u) sat |= bit;                        // Field: any emission of that path (row_matcher.go:511-516)
                if (eq && kind == 2u && q == Q_LEAF) leaf_mask |= bit;   // FieldToken: this leaf's words may complete the pair
            }
            if (kind != 0u) {                                            // conditions with a token: compare words
                const bool heq = is_word && e[4] == h[0] && e[5] == h[1] && e[6] == h[2] && e[7] == h[3];
                const bool eq = heq && e[9] == fp;
                collided |= heq && !eq;
                if (eq && (kind == 1u || (leaf_mask & bit))) sat |= bit; // Token anywhere; FieldToken only under its own path
            }
        }
        if constexpr (RANGE) {
            if (q == Q_LEAF) nl.open(w.st == S_NUM && num_listen);       // the literal's first byte is fed after this request
        }
    }
    if constexpr (RANGE) {
        decide_number(nl, nl.on, conds, a.n_conds, leaf_mask, sat, num_fail);             // the row's last number
        if (num_fail && res == R_DONE) res = R_FAIL;
    }
    if constexpr (REGEX) {
        rx.close();
        const lds_u32 *hdr = (const lds_u32 *)rx.tab;
        for (uint32_t j = 0; j < x.n_rx; ++j)
            if ((rx.sat >> j) & 1u) sat |= 1ULL << (hdr[4 * j + 1] >> 16);
        if (rx_over && res == R_DONE) res = R_FAIL;
    }
    if constexpr (SUB) {
        for (uint32_t c = 0; c < a.n_conds; ++c) {                       // uniform loop
            const uint32_t rec = (uint32_t)conds[c * kMatchCondWords + 10];
            if (RANGE && (rec & 0xFFu) == 6u) continue;                  // a range condition's record holds flags where a needle's place is
            if ((rec & 0xFFu) >= 4u && ((((rec >> 8) & 1u) ? sl.h1 : sl.h0) >> ((rec >> 16) & 63u)) & 1ULL) sat |= 1ULL << c;
        }
        if (sl.fail && res == R_DONE) res = R_FAIL;                      // a rune the lower table cannot decide: the host's ToLower does
    }
    if constexpr (WIDE) {
        // nothing is evaluated here: the flags and what became of the row go to device memory for k_eval_row_programs
        if (collided && res == R_DONE) res = R_FAIL;
        if (live) {
            wd.sat[r] = sat;
            wd.state[r] = !walk ? kRowNotWalked : res == R_DONE ? kRowDecided : kRowFallback;
        }
        if (res == R_FAIL) report_fallback(a, a.row_base + r);
        return;
    }
    if constexpr (MANY) {
        // one program per query over the same flags: the loop and the program words (LDS broadcasts) are wave-uniform, each
        // lane evaluates over its own sat, the 64 verdicts fold into one word of plane q
        if (collided && res == R_DONE) res = R_FAIL;
        const bool decided = live && res == R_DONE;
        const bool store = (threadIdx.x & 63u) == 0u && (r & ~63u) < a.n_rows;
        const lds_u32i *poff = prog + kMatchManyMaxOps;
        for (uint32_t q = 0; q < m.n_queries; ++q) {
            const uint32_t j0 = poff[q], j1 = poff[q + 1];
            uint64_t stk = 0;
            for (uint32_t j = j0; j < j1; ++j) {
                const uint32_t op = prog[j], opc = op >> 28;
                if (opc == 0u) stk = (stk << 1) | ((sat >> (op & 63u)) & 1ULL);
                else if (opc == 3u) stk = (stk << 1) | 1ULL;
                else if (opc == 4u) stk = stk << 1;
                else {
                    const uint64_t x = stk & 1ULL, y = (stk >> 1) & 1ULL;
                    stk = ((stk >> 2) << 1) | (opc == 1u ? (x & y) : (x | y));
                }
            }
            const bool verdict = (j0 == j1 ? true : (stk & 1ULL) != 0) && ((qmask >> q) & 1ULL) != 0;   // nil expression matches
            const uint64_t word = __ballot(decided && verdict);
            if (store) a.out_bits[(uint64_t)q * m.plane_words + (r >> 6)] = word;
        }
        if (res == R_FAIL) report_fallback(a, a.row_base + r);
        return;
    }
    // evalMatcherNode over the flags: one bit of stack per lane and level.  This loop and the one per query above are
    // bsh_prog::eval_program (host/row_program.hpp) written out: called as a function from here, the same evaluator re-schedules the
    // WALK of the eight kernels that end in it (k_match_rows 1.78 ms against 1.77 ms, profiles/walker_refactor.txt).  A change to the
    // opcode contract goes to the header, its CPU check and these two loops.
    uint64_t stk = 0;
    for (uint32_t j = 0; j < a.n_ops; ++j) {
        const uint32_t op = prog[j], opc = op >> 28;
        if (opc == 0u) stk = (stk << 1) | ((sat >> (op & 63u)) & 1ULL);
        else if (opc == 3u) stk = (stk << 1) | 1ULL;
        else if (opc == 4u) stk = stk << 1;
        else {
            const uint64_t x = stk & 1ULL, y = (stk >> 1) & 1ULL;
            stk = ((stk >> 2) << 1) | (opc == 1u ? (x & y) : (x | y));
        }
    }
    const bool verdict = a.n_ops == 0 ? true : (stk & 1ULL) != 0;        // nil expression matches every row
    if (collided && res == R_DONE) res = R_FAIL;
    const uint64_t word = __ballot(live && res == R_DONE && verdict);
    if ((threadIdx.x & 63u) == 0u && (r & ~63u) < a.n_rows) a.out_bits[r >> 6] = word;
    if (res == R_FAIL) report_fallback(a, a.row_base + r);
}

__global__ __launch_bounds__(kIngestThreads) void k_match_rows(const MatchArgs a) { match_rows_body<false>(a, RxArgs{}, TokDefault{}); }
// Field / Token / FieldToken and FieldRegex conditions; dynamic LDS kMatchLdsBytes + the table blob (<= kRxLdsCap)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex(const MatchArgs a, const RxArgs x) { match_rows_body<true>(a, x, TokDefault{}); }
// the same two under a separator-family tokenizer spec (bsg_match_rows_tok; regex conditions read the leaf text, not its words)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_tok(const MatchArgs a, const TokSpec t) { match_rows_body<false>(a, RxArgs{}, TokSpecP{t}); }
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_tok(const MatchArgs a, const RxArgs x, const TokSpec t)
{
    match_rows_body<true>(a, x, TokSpecP{t});
}
// ... and under a spec with an n-gram width (TokGramP): Token and FieldToken conditions compare a row's n-rune windows
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_gram(const MatchArgs a, const TokSpec t) { match_rows_body<false>(a, RxArgs{}, TokGramP(t)); }
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_gram(const MatchArgs a, const RxArgs x, const TokSpec t)
{
    match_rows_body<true>(a, x, TokGramP(t));
}
// a batch of queries over one table of Field / Token / FieldToken conditions; dynamic LDS kMatchManyLdsBytes
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many(const MatchArgs a, const MatchManyArgs m)
{
    match_rows_body<false, TokDefault, true>(a, RxArgs{}, TokDefault{}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_tok(const MatchArgs a, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokSpecP, true>(a, RxArgs{}, TokSpecP{t}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_gram(const MatchArgs a, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokGramP, true>(a, RxArgs{}, TokGramP(t), m);
}
// a batch of queries with FieldRegex conditions in the table; dynamic LDS kMatchManyLdsBytes + the table blob (<= kRxManyLdsCap)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex(const MatchArgs a, const RxArgs x, const MatchManyArgs m)
{
    match_rows_body<true, TokDefault, true, kRxManyActive>(a, x, TokDefault{}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_tok(const MatchArgs a, const RxArgs x, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokSpecP, true, kRxManyActive>(a, x, TokSpecP{t}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_gram(const MatchArgs a, const RxArgs x, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokGramP, true, kRxManyActive>(a, x, TokGramP(t), m);
}

// Field / Token / FieldToken and Substring / FieldSubstring conditions (bsg_match_rows_substr / bsg_match_rows_many_substr); dynamic
// LDS kMatchSubLdsBytes / kMatchManySubLdsBytes
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_substr(const MatchArgs a, const SubArgs sb)
{
    match_rows_body<false, TokDefault, false, kRxActive, false, true>(a, RxArgs{}, TokDefault{}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_substr_tok(const MatchArgs a, const SubArgs sb, const TokSpec t)
{
    match_rows_body<false, TokSpecP, false, kRxActive, false, true>(a, RxArgs{}, TokSpecP{t}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_substr_gram(const MatchArgs a, const SubArgs sb, const TokSpec t)
{
    match_rows_body<false, TokGramP, false, kRxActive, false, true>(a, RxArgs{}, TokGramP(t), MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_substr(const MatchArgs a, const SubArgs sb, const MatchManyArgs m)
{
    match_rows_body<false, TokDefault, true, kRxActive, false, true>(a, RxArgs{}, TokDefault{}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_substr_tok(const MatchArgs a, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokSpecP, true, kRxActive, false, true>(a, RxArgs{}, TokSpecP{t}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_substr_gram(const MatchArgs a, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokGramP, true, kRxActive, false, true>(a, RxArgs{}, TokGramP(t), m, MatchWideArgs{}, sb);
}
// ... and with FieldRegex conditions in the same table (bsg_match_rows_regex_substr / bsg_match_rows_many_regex_substr); dynamic LDS
// kMatchSubLdsBytes / kMatchManySubLdsBytes + the table blob (<= kRxSubLdsCap / kRxManySubLdsCap)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr(const MatchArgs a, const RxArgs x, const SubArgs sb)
{
    match_rows_body<true, TokDefault, false, kRxActive, false, true>(a, x, TokDefault{}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const TokSpec t)
{
    match_rows_body<true, TokSpecP, false, kRxActive, false, true>(a, x, TokSpecP{t}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const TokSpec t)
{
    match_rows_body<true, TokGramP, false, kRxActive, false, true>(a, x, TokGramP(t), MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m)
{
    match_rows_body<true, TokDefault, true, kRxManyActive, false, true>(a, x, TokDefault{}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokSpecP, true, kRxManyActive, false, true>(a, x, TokSpecP{t}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokGramP, true, kRxManyActive, false, true>(a, x, TokGramP(t), m, MatchWideArgs{}, sb);
}

// Field / Token / FieldToken and FieldRange conditions (bsg_match_rows_range / bsg_match_rows_many_range); dynamic LDS kMatchLdsBytes /
// kMatchManyLdsBytes, as the plain walkers
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_range(const MatchArgs a)
{
    match_rows_body<false, TokDefault, false, kRxActive, false, false, true>(a, RxArgs{}, TokDefault{});
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_range_tok(const MatchArgs a, const TokSpec t)
{
    match_rows_body<false, TokSpecP, false, kRxActive, false, false, true>(a, RxArgs{}, TokSpecP{t});
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_range_gram(const MatchArgs a, const TokSpec t)
{
    match_rows_body<false, TokGramP, false, kRxActive, false, false, true>(a, RxArgs{}, TokGramP(t));
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_range(const MatchArgs a, const MatchManyArgs m)
{
    match_rows_body<false, TokDefault, true, kRxActive, false, false, true>(a, RxArgs{}, TokDefault{}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_range_tok(const MatchArgs a, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokSpecP, true, kRxActive, false, false, true>(a, RxArgs{}, TokSpecP{t}, m);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_range_gram(const MatchArgs a, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<false, TokGramP, true, kRxActive, false, false, true>(a, RxArgs{}, TokGramP(t), m);
}

// Kinds 0-6 in one table (bsg_match_rows_regex_substr_range / bsg_match_rows_many_regex_substr_range): the DFAs, the needles and the number
// parser fed by one walk.  NumLane adds no LDS, so the bytes and the blob caps are the regex_substr instances': dynamic LDS
// kMatchSubLdsBytes / kMatchManySubLdsBytes + the table blob (<= kRxSubLdsCap / kRxManySubLdsCap).  One family serves every mix of the
// three sides beside a range condition: a table without a needle brings an all-zero needle table (start = any = 0), one without a regex
// condition n_rx = n_words = 0.
static_assert(2u * (kMatchSubLdsBytes + kRxSubLdsCap) <= 160u * 1024u && 2u * (kMatchManySubLdsBytes + kRxManySubLdsCap) <= 160u * 1024u,
              "k_match_rows_regex_substr_range and k_match_rows_many_regex_substr_range keep two workgroups per CU as their regex_substr siblings");
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr_range(const MatchArgs a, const RxArgs x, const SubArgs sb)
{
    match_rows_body<true, TokDefault, false, kRxActive, false, true, true>(a, x, TokDefault{}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr_range_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const TokSpec t)
{
    match_rows_body<true, TokSpecP, false, kRxActive, false, true, true>(a, x, TokSpecP{t}, MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_regex_substr_range_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const TokSpec t)
{
    match_rows_body<true, TokGramP, false, kRxActive, false, true, true>(a, x, TokGramP(t), MatchManyArgs{}, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr_range(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m)
{
    match_rows_body<true, TokDefault, true, kRxManyActive, false, true, true>(a, x, TokDefault{}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr_range_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokSpecP, true, kRxManyActive, false, true, true>(a, x, TokSpecP{t}, m, MatchWideArgs{}, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_many_regex_substr_range_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchManyArgs m, const TokSpec t)
{
    match_rows_body<true, TokGramP, true, kRxManyActive, false, true, true>(a, x, TokGramP(t), m, MatchWideArgs{}, sb);
}

// the storing walker (bsg_match_rows_wide): plain / regex x default / spec / n-gram tokenizer; dynamic LDS kMatchWideLdsBytes (+ the table
// blob, <= kRxWideLdsCap)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store(const MatchArgs a, const MatchWideArgs wd)
{
    match_rows_body<false, TokDefault, false, kRxActive, true>(a, RxArgs{}, TokDefault{}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_tok(const MatchArgs a, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokSpecP, false, kRxActive, true>(a, RxArgs{}, TokSpecP{t}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex(const MatchArgs a, const RxArgs x, const MatchWideArgs wd)
{
    match_rows_body<true, TokDefault, false, kRxActive, true>(a, x, TokDefault{}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_tok(const MatchArgs a, const RxArgs x, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokSpecP, false, kRxActive, true>(a, x, TokSpecP{t}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_gram(const MatchArgs a, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokGramP, false, kRxActive, true>(a, RxArgs{}, TokGramP(t), MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_gram(const MatchArgs a, const RxArgs x, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokGramP, false, kRxActive, true>(a, x, TokGramP(t), MatchManyArgs{}, wd);
}

// ... with the number consumer (bsg_match_rows_wide_range): kinds 0, 1, 2, 6; dynamic LDS kMatchWideLdsBytes, as k_match_rows_store.  A range
// condition listens on a leaf only where the row's set lists a query that uses it (the set's condition mask, as the regex conditions).
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_range(const MatchArgs a, const MatchWideArgs wd)
{
    match_rows_body<false, TokDefault, false, kRxActive, true, false, true>(a, RxArgs{}, TokDefault{}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_range_tok(const MatchArgs a, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokSpecP, false, kRxActive, true, false, true>(a, RxArgs{}, TokSpecP{t}, MatchManyArgs{}, wd);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_range_gram(const MatchArgs a, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokGramP, false, kRxActive, true, false, true>(a, RxArgs{}, TokGramP(t), MatchManyArgs{}, wd);
}

// ... with the substring consumer (bsg_match_rows_wide_substr): kinds 0, 1, 2, 4, 5; dynamic LDS kMatchWideSubLdsBytes.  Every needle
// listens on every walked row (needles are not gated by the set's condition mask).
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_substr(const MatchArgs a, const SubArgs sb, const MatchWideArgs wd)
{
    match_rows_body<false, TokDefault, false, kRxActive, true, true>(a, RxArgs{}, TokDefault{}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_substr_tok(const MatchArgs a, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokSpecP, false, kRxActive, true, true>(a, RxArgs{}, TokSpecP{t}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_substr_gram(const MatchArgs a, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<false, TokGramP, false, kRxActive, true, true>(a, RxArgs{}, TokGramP(t), MatchManyArgs{}, wd, sb);
}
// ... and with both consumers: kinds 0-5; dynamic LDS kMatchWideSubLdsBytes + the table blob (<= kRxWideSubLdsCap)
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd)
{
    match_rows_body<true, TokDefault, false, kRxActive, true, true>(a, x, TokDefault{}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokSpecP, false, kRxActive, true, true>(a, x, TokSpecP{t}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokGramP, false, kRxActive, true, true>(a, x, TokGramP(t), MatchManyArgs{}, wd, sb);
}
// ... and with all three (bsg_match_rows_wide_regex_substr_range): kinds 0-6.  NumLane adds no LDS, so the bytes and the blob cap are the
// regex_substr instances': dynamic LDS kMatchWideSubLdsBytes + the table blob (<= kRxWideSubLdsCap).  One family serves every mix of the
// three sides beside a range condition: the needle table always sits at kMatchWideLdsBytes (all zero without a needle: start = any = 0),
// the blob behind it (n_rx = n_words = 0 without a regex condition), and the blob's cap is the same with a needle and without one.
static_assert(2u * (kMatchWideSubLdsBytes + kRxWideSubLdsCap) <= 160u * 1024u && 3u * (kMatchWideSubLdsBytes + kRxWideSubLdsCap) > 160u * 1024u,
              "k_match_rows_store_regex_substr_range keeps two workgroups per CU with a blob at the cap, as its regex_substr sibling");
static_assert(3u * kMatchWideSubLdsBytes <= 160u * 1024u,
              "k_match_rows_store_regex_substr_range keeps three workgroups per CU without a blob, as k_match_rows_store_substr");
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr_range(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd)
{
    match_rows_body<true, TokDefault, false, kRxActive, true, true, true>(a, x, TokDefault{}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr_range_tok(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokSpecP, false, kRxActive, true, true, true>(a, x, TokSpecP{t}, MatchManyArgs{}, wd, sb);
}
__global__ __launch_bounds__(kIngestThreads) void k_match_rows_store_regex_substr_range_gram(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd, const TokSpec t)
{
    match_rows_body<true, TokGramP, false, kRxActive, true, true, true>(a, x, TokGramP(t), MatchManyArgs{}, wd, sb);
}

// The programs of the listed (set, query) pairs over the stored flags.  Wave w of the grid owns item w: one 64-row tile of one set
// and up to kItemPairs of the set's pairs.  Everything but sat / state / the ballot is wave-uniform and read through the constant
// address space (items, pairs, prog_off and prog are written by the host before the launch, never by a kernel): scalar loads, the
// loop bounds in SGPRs, no LDS.  Lane 0 stores the pair's word of the tile with a vector store.
constexpr uint32_t kRowEvalThreads = 256;
// make_term(row, live) gives the lane's TERM reader: how it reads flag c of its row.  The reader is ONE object for all of the item's
// pairs and goes to eval_program as an lvalue: what it keeps (k_eval_row_programs_w: the last word loaded) lasts from pair to pair.
template <class MAKE>
__device__ __forceinline__ void eval_row_programs_body(const RowEvalArgs &e, MAKE &&make_term)
{
    typedef const __attribute__((address_space(4))) uint64_t c64;
    typedef const __attribute__((address_space(4))) uint32_t c32;
    const uint32_t it = blockIdx.x * (kRowEvalThreads / 64u) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (it >= e.n_items) return;
    c64 *iw = (c64 *)(uintptr_t)(e.items + it);
    const uint64_t out0 = iw[0], w1 = iw[1], w2 = iw[2], w3 = iw[3];
    const uint32_t row0 = (uint32_t)w1, n_rows = (uint32_t)(w1 >> 32), pair0 = (uint32_t)w2, pair1 = (uint32_t)(w2 >> 32), stride = (uint32_t)w3;
    c32 *pairs = (c32 *)(uintptr_t)e.pairs, *poff = (c32 *)(uintptr_t)e.prog_off, *prog = (c32 *)(uintptr_t)e.prog;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = lane < n_rows;
    auto term = make_term(row0 + lane, live);
    const bool decided = live && e.state[row0 + lane] == kRowDecided;
    for (uint32_t p = pair0; p < pair1; ++p) {
        const uint32_t q = pairs[p];
        const bool verdict = bsh_prog::eval_program(prog, poff[q], poff[q + 1], term);   // every lane: the program words stay wave-uniform
        const uint64_t word = __ballot(decided && verdict);
        if (lane == 0u) e.out[out0 + (uint64_t)(p - pair0) * stride] = word;
    }
}
// the row's one flag word, loaded once
__global__ __launch_bounds__(kRowEvalThreads) void k_eval_row_programs(const RowEvalArgs e)
{
    eval_row_programs_body(e, [&](uint32_t row, bool live) {
        return [sat = live ? e.sat[row] : 0ull](uint32_t c) { return (sat >> (c & 63u)) & 1ULL; };
    });
}

// ---- the part's words as tagged row lists (bsg_match_rows_wide_rows) ----
// Three passes over what k_eval_row_programs left in RowEvalArgs::out, a wave per pair of the part in the first and the last:
//   k_pair_sizes   the pair's header over the part's rows of its set and its payload's u32 (host/wide_plan.hpp pair_header)
//   k_pair_scan_*  the exclusive u64 prefix of the sizes over the part's pairs: block sums, their scan (one workgroup that walks
//                  them kPairScanWidth at a time with a carry: any number of blocks), then each block's own scan behind its base
//   k_pair_write   LIST: set-relative row indices, ascending; DENSE: the words copied as u32
// Device memory: the payload scratch is sized at its bound, 2 u32 per result word (what RowEvalArgs::out takes once more), plus 20
// bytes per pair (header, size, offset), 8 per kPairScanWidth pairs and 24 per set of the part.  Only the headers and the payload's
// first `total` u32 travel back.
constexpr uint32_t kPairNone = 0, kPairAll = 1, kPairList = 2, kPairDense = 3;
constexpr uint32_t kPairThreads = 256;         // four waves, a pair each
constexpr uint32_t kPairScanWidth = 256;       // pairs per workgroup of the scan, one per thread
struct PairSetDesc {                           // host/wide_plan.hpp PairSet
    uint64_t word0;                            // where the set's first pair's words begin in `words`
    uint32_t pair0, rows, tile0, pad;          // its first pair, the part's rows of it, the set's tile they begin at
};
struct PairRowsArgs {
    const PairSetDesc *sets;                   // [n_sets + 1], the last one closes the table (pair0 = n_pairs)
    const uint64_t *words;                     // the part's result words
    uint32_t *hdr;                             // [n_pairs]
    uint64_t *size;                            // [n_pairs] u32 of payload
    uint64_t *off;                             // [n_pairs + 1] their exclusive prefix, then the total
    uint64_t *block_sum;                       // [ceil(n_pairs / kPairScanWidth)]
    uint32_t *payload;
    uint32_t n_pairs, n_sets;
};

// the local set of pair lp: the last one whose pair0 is <= lp (sets without pairs share their pair0 with the next one)
__device__ __forceinline__ uint32_t pair_set_of(const PairSetDesc *sets, uint32_t n_sets, uint32_t lp)
{
    uint32_t lo = 0, hi = n_sets;              // sets[lo].pair0 <= lp < sets[hi].pair0
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sets[mid].pair0 <= lp) lo = mid; else hi = mid;
    }
    return lo;
}

template <class T>
__device__ __forceinline__ T wave_inclusive_sum(T v, uint32_t lane)
{
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_sizes(const PairRowsArgs a)
{
    const uint32_t lp = blockIdx.x * (kPairThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (lp >= a.n_pairs) return;
    const PairSetDesc sd = a.sets[pair_set_of(a.sets, a.n_sets, lp)];
    const uint32_t T = (sd.rows + 63u) / 64u;
    const uint64_t *w = a.words + sd.word0 + (uint64_t)(lp - sd.pair0) * T;
    uint32_t c = 0;
    for (uint32_t t = lane; t < T; t += 64u) c += (uint32_t)__popcll(w[t]);
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, (int)o, 64);
    if (lane == 0u) {
        const uint32_t tag = c == 0u ? kPairNone : c == sd.rows ? kPairAll : c < 2u * T ? kPairList : kPairDense;
        a.hdr[lp] = tag << 30 | (tag == kPairList ? c : 0u);
        a.size[lp] = tag == kPairList ? (uint64_t)c : tag == kPairDense ? 2ull * T : 0ull;
    }
}

// the inclusive prefix of one value per thread over the workgroup's kPairScanWidth threads; *total = their sum
__device__ __forceinline__ uint64_t block_inclusive_sum(uint64_t v, uint64_t *wave_total, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = wave_inclusive_sum(v, lane);
    if (lane == 63u) wave_total[wave] = incl;
    __syncthreads();
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPairScanWidth / 64u; ++k) {
        if (k < wave) incl += wave_total[k];
        sum += wave_total[k];
    }
    __syncthreads();                           // wave_total may be written again
    *total = sum;
    return incl;
}

__global__ __launch_bounds__(kPairScanWidth) void k_pair_scan_sums(const PairRowsArgs a)
{
    __shared__ uint64_t wave_total[kPairScanWidth / 64u];
    const uint32_t i = blockIdx.x * kPairScanWidth + threadIdx.x;
    uint64_t total;
    (void)block_inclusive_sum(i < a.n_pairs ? a.size[i] : 0ull, wave_total, &total);
    if (threadIdx.x == 0u) a.block_sum[blockIdx.x] = total;
}

// ONE workgroup: block_sum [n_blocks] becomes its own exclusive prefix, off[n_pairs] the total
__global__ __launch_bounds__(kPairScanWidth) void k_pair_scan_blocks(const PairRowsArgs a, const uint32_t n_blocks)
{
    __shared__ uint64_t wave_total[kPairScanWidth / 64u];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kPairScanWidth) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < n_blocks ? a.block_sum[b] : 0ull;
        uint64_t total;
        const uint64_t incl = block_inclusive_sum(v, wave_total, &total);
        if (b < n_blocks) a.block_sum[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0u) a.off[a.n_pairs] = carry;
}

__global__ __launch_bounds__(kPairScanWidth) void k_pair_scan_apply(const PairRowsArgs a)
{
    __shared__ uint64_t wave_total[kPairScanWidth / 64u];
    const uint32_t i = blockIdx.x * kPairScanWidth + threadIdx.x;
    const uint64_t v = i < a.n_pairs ? a.size[i] : 0ull;
    uint64_t total;
    const uint64_t incl = block_inclusive_sum(v, wave_total, &total);
    if (i < a.n_pairs) a.off[i] = a.block_sum[blockIdx.x] + incl - v;
}

__global__ __launch_bounds__(kPairThreads) void k_pair_write(const PairRowsArgs a)
{
    const uint32_t lp = blockIdx.x * (kPairThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (lp >= a.n_pairs) return;
    const uint32_t tag = a.hdr[lp] >> 30;
    if (tag != kPairList && tag != kPairDense) return;
    const PairSetDesc sd = a.sets[pair_set_of(a.sets, a.n_sets, lp)];
    const uint32_t T = (sd.rows + 63u) / 64u;
    const uint64_t *w = a.words + sd.word0 + (uint64_t)(lp - sd.pair0) * T;
    uint32_t *out = a.payload + a.off[lp];     // size[lp] u32: c of a LIST (the bits of w), 2T of a DENSE pair
    if (tag == kPairDense) {
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(w);
        for (uint32_t i = lane; i < 2u * T; i += 64u) out[i] = w32[i];
        return;
    }
    uint32_t base = 0;                         // the bits of the rounds before
    for (uint32_t t0 = 0; t0 < T; t0 += 64u) {
        const uint32_t t = t0 + lane;
        uint64_t x = t < T ? w[t] : 0ull;
        const uint32_t cnt = (uint32_t)__popcll(x), incl = wave_inclusive_sum(cnt, lane);
        uint32_t at = base + incl - cnt;
        for (; x; x &= x - 1) out[at++] = (sd.tile0 + t) * 64u + (uint32_t)__builtin_ctzll(x);
        base += (uint32_t)__shfl((int)incl, 63, 64);
    }
}

}  // namespace bsg
