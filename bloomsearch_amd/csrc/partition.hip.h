// partition.hip.h — the rows of a streaming ingest partitioned ON THE DEVICE by the text of one top-level member (the engine's
// PartitionField, the stand-in for the reference's PartitionFunc, ingest.go:364-367), gfx950.
//
// The rule (include/bloomgpu.h; it restates host/json.hpp validate_object_row): the FIRST top-level member whose key
// equals the name byte for byte counts — later members with that key are never looked at, the scanner stops at the end of the found
// member's value.  A string value gives the bytes between its quotes, a number its raw literal as written (no arithmetic), true and
// false their four or five bytes; null, an object, an array or no such member give the empty text.  Equal text is the same
// partition whatever the JSON type.  Rows the device does not decide (handed back, their set is kPkeyUndecided): a string value that
// holds a backslash, a text of more than kPkeyMaxKey bytes, and a top-level key with a backslash that the scanner meets — it meets
// one only before the member is found or when the member is never found, and such a key could decode to the name.
//
// k_partition_rows: one lane scans one row (partition_scan_row: container depth as a counter, string and escape state, the key
// narrowed byte by byte against the one name in LDS, the SWAR run skip of minmax.hip.h inside strings nobody compares), hashes the
// text (FNV-1a, folded to 31 bits) and looks it up in the ingest's key dictionary: an open-addressing table (tag, set, offset and
// length into a pool of key bytes) the HOST owns and extends; kernels only read it.  A hit is taken only after the bytes compare
// equal.  A decided row whose text is not in the dictionary claims a slot of the call's pending table by compare-and-swap on the tag
// and records the lowest row index that met the slot with an atomic min; two texts with one tag share a slot.  The host reads the
// claimed slots (a few per batch), takes each slot's text from its own copy of that lowest row and extends the dictionary.
// k_partition_assign resolves the rows still unassigned against the extended dictionary, again with the byte compare, and lets the
// rows that still miss (the other text of a shared tag, a text that found the pending table full) claim again: rounds until no row
// claims.  Every text's lowest row is exact: all of a text's rows stay unassigned until the text is in the dictionary, and a slot's
// lowest row is a row of the text taken from it.
//
// Reads: as minmax.hip.h — the 8-byte words that hold [row_off[r], row_off[r + 1]) plus one word of look-ahead; the text's bytes lie
// inside the row.  Writes: the row's own PkeyRow and set, the pending table's slots (index < kPkeyPendingSlots by masking).
//
// The per-row scanner and the hash are plain C++ shared by host and device: tests/partition_scan_check.cpp runs the same functions on
// the CPU under the sanitizers, over the shapes, every alignment and every truncation.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#include "ingest.hip.h"
#define BSG_PT_HD __host__ __device__ __forceinline__
#else
#define BSG_PT_HD inline
#endif

namespace bsg {

constexpr uint32_t kPkeyMaxName = 64;          // bloomgpu.h BSG_PARTITION_MAX_NAME
constexpr uint32_t kPkeyMaxKey = 128;          // bloomgpu.h BSG_PARTITION_MAX_KEY
constexpr uint32_t kPkeyPendingSlots = 256;    // bloomgpu.h BSG_PARTITION_PENDING_SLOTS (a power of two)
constexpr uint32_t kPkeyUndecided = 0xFFFFFFFFu;   // bloomgpu.h BSG_SET_UNDECIDED
constexpr uint32_t kPkeyNew = 0xFFFFFFFEu;     // decided, its text not in the dictionary (yet): never leaves the library
constexpr uint32_t kPkeyProvisional = 0x80000000u;  // | index among the call's new keys: a dictionary entry whose set is not numbered yet
constexpr int kPkeyThreads = 256;

enum : uint32_t { PT_STR = 1u, PT_ESC = 2u, PT_KEY = 4u, PT_EXPECT_KEY = 8u, PT_VALUE = 16u, PT_MATCH = 32u };

struct PkeyScan {
    uint32_t undecided;             // 1: the row is handed back
    uint64_t pos;                   // the text: bytes [pos, pos + len) of the buffer
    uint32_t len;
};

// One row: bytes [pos, end) of the buffer `chunks` holds as aligned 8-byte words (readable up to the word behind the one with the
// row's last byte).  name: the partition field, 1 <= name_len <= kPkeyMaxName.
BSG_PT_HD PkeyScan partition_scan_row(const uint64_t *chunks, uint64_t pos, uint64_t end, const uint8_t *name, uint32_t name_len)
{
    uint32_t st = 0, depth = 0, cand = 0, klen = 0;
    if (pos >= end) return PkeyScan{0u, pos, 0u};
    uint64_t ci = pos >> 3;
    uint64_t cur = chunks[ci], nxt = chunks[ci + 1];     // one word ahead: its latency hides behind the bytes of this one
    while (pos < end) {
        while ((pos >> 3) != ci) { ++ci; cur = nxt; nxt = chunks[ci + 1]; }      // (pos < end: word ci holds a byte of the row)
        const uint32_t c = (uint32_t)(cur >> ((pos & 7u) * 8u)) & 0xFFu;
        if (st & PT_STR) {
            if (!(st & PT_ESC) && (!(st & PT_KEY) || cand == 0u)) {
                // most bytes of a row lie inside strings nobody compares: the run up to the word's first quote or backslash at once
                const uint64_t w = cur >> ((pos & 7u) * 8u);
                const uint64_t q = w ^ 0x2222222222222222ULL, b = w ^ 0x5C5C5C5C5C5C5C5CULL;
                const uint64_t hit = ((q - 0x0101010101010101ULL) & ~q & 0x8080808080808080ULL) | ((b - 0x0101010101010101ULL) & ~b & 0x8080808080808080ULL);
                uint64_t n = hit ? (uint64_t)(__builtin_ctzll(hit) >> 3) : 8u;
                const uint64_t in_word = 8u - (pos & 7u);
                if (n > in_word) n = in_word;
                if (n > end - pos) n = end - pos;
                if (n) { pos += n; continue; }
            }
            if (st & PT_ESC) st &= ~PT_ESC;
            else if (c == '\\') {
                if (st & PT_KEY) return PkeyScan{1u, pos, 0u};         // a top-level key that could decode to the name
                st |= PT_ESC;
            }
            else if (c == '"') {
                if ((st & PT_KEY) && cand && klen == name_len) st |= PT_MATCH;
                st &= ~(PT_STR | PT_KEY);
            } else if (st & PT_KEY) {
                if (klen >= name_len || name[klen] != c) cand = 0u;   // klen < name_len <= 64
                ++klen;
            }
            ++pos;
            continue;
        }
        if (c == ' ' || c == '\t' || c == '\n' || c == '\r') { ++pos; continue; }
        if (st & PT_VALUE) {                                    // the first byte of a top-level member's value
            st &= ~PT_VALUE;
            if (st & PT_MATCH) {
                // the member: its text, and nothing behind it is looked at
                uint64_t p = pos, stop = end;
                if (c == '"') {
                    const uint64_t t0 = ++p;
                    if (end - t0 > (uint64_t)kPkeyMaxKey + 1u) stop = t0 + kPkeyMaxKey + 1u;   // a longer text is handed back wherever it ends
                    for (; p < stop; ++p) {
                        while ((p >> 3) != ci) { ++ci; cur = nxt; nxt = chunks[ci + 1]; }
                        const uint32_t v = (uint32_t)(cur >> ((p & 7u) * 8u)) & 0xFFu;
                        if (v == '\\') return PkeyScan{1u, t0, 0u};
                        if (v == '"') return PkeyScan{0u, t0, (uint32_t)(p - t0)};
                    }
                    return PkeyScan{1u, t0, 0u};                // no closing quote within kPkeyMaxKey bytes (or within the row)
                }
                if (c == '-' || c - (uint32_t)'0' <= 9u) {
                    if (end - pos > (uint64_t)kPkeyMaxKey + 1u) stop = pos + kPkeyMaxKey + 1u;
                    for (; p < stop; ++p) {
                        while ((p >> 3) != ci) { ++ci; cur = nxt; nxt = chunks[ci + 1]; }
                        const uint32_t v = (uint32_t)(cur >> ((p & 7u) * 8u)) & 0xFFu;
                        if (!(v - (uint32_t)'0' <= 9u || v == '.' || v == '-' || v == '+' || (v | 0x20u) == 'e')) break;
                    }
                    const uint32_t len = (uint32_t)(p - pos);
                    return len > kPkeyMaxKey ? PkeyScan{1u, pos, 0u} : PkeyScan{0u, pos, len};
                }
                const uint64_t left = end - pos;
                if (c == 't') return PkeyScan{0u, pos, (uint32_t)(left < 4u ? left : 4u)};
                if (c == 'f') return PkeyScan{0u, pos, (uint32_t)(left < 5u ? left : 5u)};
                return PkeyScan{0u, pos, 0u};                   // null, an object, an array
            }
        }
        if (c == '"') {
            st |= PT_STR;
            if (depth == 1u && (st & PT_EXPECT_KEY)) { st = (st & ~PT_EXPECT_KEY) | PT_KEY; cand = 1u; klen = 0; }
        }
        else if (c == '{') { if (++depth == 1u) st |= PT_EXPECT_KEY; }
        else if (c == '[') ++depth;
        else if (c == '}' || c == ']') { if (depth) --depth; }
        else if (c == ',') { if (depth == 1u) st |= PT_EXPECT_KEY; }
        else if (c == ':') { if (depth == 1u) st |= PT_VALUE; }
        ++pos;
    }
    return PkeyScan{0u, end, 0u};                              // no such member
}

// The dictionary tag of a text: FNV-1a over its bytes folded to 31 bits, masked (the lab key leaves 2 bits), bit 31 set so that no
// tag is 0 (an empty slot).
BSG_PT_HD uint64_t partition_hash_step(uint64_t h, uint32_t c) { return (h ^ c) * 0x100000001B3ULL; }
constexpr uint64_t kPkeyHashSeed = 0xCBF29CE484222325ULL;
BSG_PT_HD uint32_t partition_tag(uint64_t h, uint32_t mask) { return (((uint32_t)(h >> 32) ^ (uint32_t)h) & mask & 0x7FFFFFFFu) | 0x80000000u; }
BSG_PT_HD uint32_t partition_tag_bytes(const uint8_t *p, uint32_t len, uint32_t mask)
{
    uint64_t h = kPkeyHashSeed;
    for (uint32_t i = 0; i < len; ++i) h = partition_hash_step(h, p[i]);
    return partition_tag(h, mask);
}

struct PkeyDictEntry { uint32_t tag, set, off, len; };       // tag 0: empty.  Linear probing from tag & mask.
struct PkeyPending { uint32_t tag, first_row; };             // tag 0: unclaimed; first_row starts at 0xFFFFFFFF
struct PkeyRow { uint32_t off, len, tag; };                   // a decided row's text (offset from the row's first byte) and tag

#ifdef __HIPCC__
struct PkeyArgs {
    const uint8_t *rows;            // as IngestArgs
    const uint64_t *row_off;
    const PkeyDictEntry *dict;      // dict_mask + 1 slots, at least one of them empty
    const uint8_t *pool;
    PkeyPending *pending;           // [kPkeyPendingSlots]
    PkeyRow *row_key;               // [n_rows]
    uint32_t *set_of_row;           // [n_rows]
    uint32_t dict_mask;
    uint32_t hash_mask;
    uint32_t row_first, row_end;
};

struct PkeyName { uint8_t name[kPkeyMaxName]; uint32_t len; };   // by value in the kernel arguments

__device__ __forceinline__ uint32_t part_byte(const uint64_t *chunks, uint64_t p) { return (uint32_t)(chunks[p >> 3] >> ((p & 7u) * 8u)) & 0xFFu; }

// the set of the text [t0, t0 + len) with this tag, or kPkeyNew
__device__ __forceinline__ uint32_t part_lookup(const PkeyArgs &a, const uint64_t *chunks, uint64_t t0, uint32_t len, uint32_t tag)
{
    for (uint32_t i = tag & a.dict_mask, n = 0; n <= a.dict_mask; i = (i + 1u) & a.dict_mask, ++n) {
        const PkeyDictEntry e = a.dict[i];
        if (e.tag == 0u) break;
        if (e.tag != tag || e.len != len) continue;
        uint32_t k = 0;
        while (k < len && a.pool[e.off + k] == part_byte(chunks, t0 + k)) ++k;      // the hash alone never decides
        if (k == len) return e.set;
    }
    return kPkeyNew;
}

// a slot for this tag in the call's pending table; a full table leaves the row to a later round
__device__ __forceinline__ void part_claim(const PkeyArgs &a, uint32_t tag, uint32_t r)
{
    for (uint32_t i = tag & (kPkeyPendingSlots - 1u), n = 0; n < kPkeyPendingSlots; i = (i + 1u) & (kPkeyPendingSlots - 1u), ++n) {
        uint32_t seen = __hip_atomic_load(&a.pending[i].tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0u) {
            uint32_t expect = 0u;
            if (__hip_atomic_compare_exchange_strong(&a.pending[i].tag, &expect, tag, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) seen = tag;
            else seen = expect;
        }
        if (seen == tag) { __hip_atomic_fetch_min(&a.pending[i].first_row, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    }
}

__global__ __launch_bounds__(kPkeyThreads) void k_partition_rows(const PkeyArgs a, const PkeyName nm)
{
    __shared__ uint8_t name[kPkeyMaxName];
    if (threadIdx.x < kPkeyMaxName) name[threadIdx.x] = nm.name[threadIdx.x];
    __syncthreads();
    const uint64_t r64 = (uint64_t)a.row_first + (uint64_t)blockIdx.x * kPkeyThreads + threadIdx.x;
    if (r64 >= a.row_end) return;
    const uint32_t r = (uint32_t)r64;
    const uint64_t *chunks = reinterpret_cast<const uint64_t *>(a.rows);
    const uint64_t pos = a.row_off[r], end = a.row_off[r + 1];
    const PkeyScan sc = partition_scan_row(chunks, pos, end, name, nm.len);
    if (sc.undecided) { a.set_of_row[r] = kPkeyUndecided; return; }
    uint64_t h = kPkeyHashSeed;
    for (uint32_t k = 0; k < sc.len; ++k) h = partition_hash_step(h, part_byte(chunks, sc.pos + k));
    const uint32_t tag = partition_tag(h, a.hash_mask);
    a.row_key[r] = PkeyRow{(uint32_t)(sc.pos - pos), sc.len, tag};
    const uint32_t set = part_lookup(a, chunks, sc.pos, sc.len, tag);
    a.set_of_row[r] = set;
    if (set == kPkeyNew) part_claim(a, tag, r);
}

// rows [row_first, row_end) once more: those still kPkeyNew against the dictionary as it is now
__global__ __launch_bounds__(kPkeyThreads) void k_partition_assign(const PkeyArgs a)
{
    const uint64_t r64 = (uint64_t)a.row_first + (uint64_t)blockIdx.x * kPkeyThreads + threadIdx.x;
    if (r64 >= a.row_end) return;
    const uint32_t r = (uint32_t)r64;
    if (a.set_of_row[r] != kPkeyNew) return;
    const PkeyRow k = a.row_key[r];
    const uint32_t set = part_lookup(a, reinterpret_cast<const uint64_t *>(a.rows), a.row_off[r] + k.off, k.len, k.tag);
    if (set != kPkeyNew) a.set_of_row[r] = set;
    else part_claim(a, k.tag, r);
}
#endif  // __HIPCC__

}  // namespace bsg
