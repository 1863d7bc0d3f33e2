// regex_groups.hpp — the arithmetic of FieldRegex conditions in a batch of queries, free of any device type: which regex
// conditions can meet on one leaf (co_active_bound), what a pattern's DFA costs in the kernel's LDS table blob (rx_table_bytes),
// which queries use a condition (user_masks), and the blob itself (build_blob / build_blob_of: layout in match.hip.h).  bsg_match_rows_regex /
// bsg_match_rows_tok / bsg_match_rows_many_regex (match_api.inc) build their tables by these functions and the engine mirror
// (engine.hpp match_rows_device_many) closes its groups by them; tests/regex_groups_check.cpp runs the same code on the CPU
// (tests/test_regex_groups.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "regex_dfa.hpp"

namespace bsh_rxg {

constexpr uint32_t kMaxRegexConds = 16;        // match.hip.h kRxMaxConds
constexpr uint32_t kSingleLdsCap = 44544;      // match.hip.h kRxLdsCap: table bytes of bsg_match_rows_regex / _tok
constexpr uint32_t kManyLdsCap = 38140;        // match.hip.h kRxManyLdsCap: table bytes of bsg_match_rows_many_regex
constexpr uint32_t kSingleSubLdsCap = 40448;   // match.hip.h kRxSubLdsCap: table bytes of bsg_match_rows_regex_substr beside a needle table
constexpr uint32_t kManySubLdsCap = 34032;     // match.hip.h kRxManySubLdsCap: the same of bsg_match_rows_many_regex_substr
constexpr uint32_t kWideSubLdsCap = 42496;     // match.hip.h kRxWideSubLdsCap: the same of bsg_match_rows_wide_substr
constexpr uint32_t kSingleSlots = 4;           // match.hip.h kRxActive: regex conditions one leaf may feed at once
constexpr uint32_t kManySlots = 4;             // match.hip.h kRxManyActive: the same in the batched kernels.  Another shipped count means
                                               // this literal and the "4" of bloomgpu.h, bloomsearch_host.h, INTEGRATION.md, bloomgpu.go and
                                               // tests/test_match_many_regex_gpu.py (SLOTS) change by hand
constexpr uint32_t kPathCap = 96;              // ingest.hip.h kPathCap: the longest path a lane keeps
constexpr uint32_t kHeaderBytes = 16, kUserMaskBytes = 8;

// a condition on field `a` sees every leaf at or under a: the leaf's path equals a or starts with a + "." (row_matcher.go hasStringPrefix)
inline bool covers(std::string_view a, std::string_view path)
{
    if (a.empty() || a.size() > path.size() || path.compare(0, a.size(), a) != 0) return false;
    return a.size() == path.size() || path[a.size()] == '.';
}

// The most regex conditions of `fields` that one leaf of any row can lie under.  Two conditions meet on a leaf only if their fields are
// equal or one is a dotted prefix of the other, and the fields covering one path form a chain; the longest member of the chain is
// covered by all of them, so the maximum over paths is reached at one of the fields.
inline uint32_t co_active_bound(const std::vector<std::string_view> &fields)
{
    uint32_t best = 0;
    for (const std::string_view f : fields) {
        uint32_t n = 0;
        for (const std::string_view a : fields) n += covers(a, f) ? 1u : 0u;
        best = std::max(best, n);
    }
    return best;
}

inline uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }

// What one regex condition adds to the table blob: its header words (and user mask in the batched blob), the class map and the
// transitions padded to 4 bytes, and its field string (a field beyond kPathCap is not stored: no decided row has such a path).
// The sum over a table's conditions, padded to 4 bytes, is the blob's size or 4 bytes above it (build_blob pads in front of a
// region, so the padding behind the last one is not spent).
inline uint32_t rx_table_bytes(uint32_t n_states, uint32_t n_classes, uint32_t field_len, bool many)
{
    return kHeaderBytes + (many ? kUserMaskBytes : 0u) + align4(256u + 2u * n_states * n_classes) + (field_len <= kPathCap ? field_len : 0u);
}

// bit q of masks[c]: program q references condition c (public postfix ops: opcode 0 = TERM, the low 28 bits its condition)
inline std::vector<uint64_t> user_masks(const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, uint32_t n_conds)
{
    std::vector<uint64_t> masks(n_conds, 0);
    for (uint32_t q = 0; q < n_queries && q < 64; ++q)
        for (uint32_t j = prog_off[q]; j < prog_off[q + 1]; ++j) {
            const uint32_t arg = prog_ops[j] & 0x0FFFFFFFu;
            if ((prog_ops[j] >> 28) == 0u && arg < n_conds) masks[arg] |= 1ull << q;
        }
    return masks;
}

enum class BlobStatus { Ok, TooMany, Pattern, OverCap };
struct BlobResult {
    BlobStatus status = BlobStatus::Ok;
    uint32_t cond = 0;                // Pattern: the condition whose pattern does not compile
    std::string err;                  // Pattern: what the compiler said
    uint32_t n_rx = 0;
    std::vector<uint32_t> estimate;   // per regex condition: rx_table_bytes of its DFA and field
};

// The LDS table blob of a table's FieldRegex conditions (kind 3), as words.  users: NULL = the single call's blob; else
// [n_conds] user masks, stored as n_rx u64 behind the header (the batched blob).  Nothing is refused silently: status says why.
// rx: the table's regex conditions, ascending; slot j of the blob is condition rx[j].
inline BlobResult build_blob_of(const uint8_t *cond_bytes, const uint32_t *cond_off, const std::vector<uint32_t> &rx, uint32_t cap, const uint64_t *users,
                                std::vector<uint32_t> &blob)
{
    BlobResult res;
    const uint32_t n_rx = res.n_rx = (uint32_t)rx.size();
    blob.clear();
    if (rx.empty()) return res;
    if (n_rx > kMaxRegexConds) { res.status = BlobStatus::TooMany; return res; }
    const size_t hdr = (size_t)n_rx * kHeaderBytes;
    std::vector<uint8_t> bytes(hdr + (users ? (size_t)n_rx * kUserMaskBytes : 0), 0);
    auto put32 = [&](size_t at, uint32_t v) { memcpy(bytes.data() + at, &v, 4); };
    bool over = false;
    for (uint32_t j = 0; j < n_rx; ++j) {
        const uint32_t c = rx[j];
        const std::string_view pat((const char *)cond_bytes + cond_off[2 * c + 1], cond_off[2 * c + 2] - cond_off[2 * c + 1]);
        bsh_rx::Dfa d;
        if (!bsh_rx::compile(pat, d, res.err)) { res.status = BlobStatus::Pattern; res.cond = c; return res; }
        res.estimate.push_back(rx_table_bytes(d.n_states, d.n_classes, cond_off[2 * c + 1] - cond_off[2 * c], users != nullptr));
        bytes.resize((bytes.size() + 3) & ~(size_t)3);
        const size_t off = bytes.size();
        if (off + 256 + d.trans.size() * 2 > cap) { over = true; break; }
        bytes.insert(bytes.end(), d.cls, d.cls + 256);
        const size_t t0 = bytes.size();
        bytes.resize(t0 + d.trans.size() * 2);
        memcpy(bytes.data() + t0, d.trans.data(), d.trans.size() * 2);
        put32((size_t)j * 16, (uint32_t)off | ((d.n_classes - 1) << 16) | (j << 24));
        put32((size_t)j * 16 + 4, (uint32_t)d.start | (c << 16));
        if (users) memcpy(bytes.data() + hdr + (size_t)j * 8, &users[c], 8);
    }
    for (uint32_t j = 0; j < n_rx && !over; ++j) {
        const uint32_t c = rx[j];
        uint32_t flen = cond_off[2 * c + 1] - cond_off[2 * c];
        // a path the device keeps is at most kPathCap bytes: a longer field is never at or above a leaf of a row it decides
        if (flen > kPathCap) flen = kPathCap + 1;
        const size_t off = bytes.size();
        if (flen <= kPathCap) bytes.insert(bytes.end(), cond_bytes + cond_off[2 * c], cond_bytes + cond_off[2 * c] + flen);
        put32((size_t)j * 16 + 8, (uint32_t)std::min<size_t>(off, 0xFFFF) | (flen << 16));
    }
    if (over || bytes.size() > cap) { res.status = BlobStatus::OverCap; return res; }
    bytes.resize((bytes.size() + 3) & ~(size_t)3);
    blob.resize(bytes.size() / 4);
    memcpy(blob.data(), bytes.data(), bytes.size());
    return res;
}
// ... of every condition of kind regex_kind (the lookup call passes build_blob_of its DISTINCT regex conditions instead)
inline BlobResult build_blob(const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds, uint32_t regex_kind,
                             uint32_t cap, const uint64_t *users, std::vector<uint32_t> &blob)
{
    std::vector<uint32_t> rx;
    for (uint32_t c = 0; c < n_conds; ++c)
        if (cond_kinds[c] == regex_kind) rx.push_back(c);
    return build_blob_of(cond_bytes, cond_off, rx, cap, users, blob);
}

}  // namespace bsh_rxg
