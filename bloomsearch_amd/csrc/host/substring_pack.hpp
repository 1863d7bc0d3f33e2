// substring_pack.hpp — what the host's substring conditions (substring.hpp) and the device call (match_api.inc bsg_match_rows_substr)
// share: a needle's limits and folding, and the packed shift-and tables the device row walker's text consumer steps
// (match.hip.h SubLane).  Text tables only: no query tree, no walker.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "text.hpp"

namespace bsh {

constexpr uint32_t kSubMaxNeedle = 64;     // bytes of a folded needle: one needle never straddles a 64-bit word of the device's state
constexpr uint32_t kSubWords = 2;          // state words per lane: 128 needle bytes per call

inline bool valid_utf8(std::string_view s)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(s.data());
    for (size_t i = 0; i < s.size();) {
        size_t w;
        const uint32_t r = decode_rune(p + i, s.size() - i, w);
        if (r == kRuneError && w == 1) return false;       // (a literal U+FFFD decodes with width 3)
        i += w;
    }
    return true;
}

inline std::string fold_text(std::string_view s, bool lower)
{
    if (!lower) return std::string(s);
    std::string out;
    out.reserve(s.size());
    append_folded_word(out, s);
    return out;
}

enum class NeedleStatus : uint8_t { Ok, Invalid, TooLong };
// a needle is non-empty valid UTF-8 of at most kSubMaxNeedle bytes after folding
inline NeedleStatus fold_needle(std::string_view needle, const Tokenizer &t, std::string &folded)
{
    if (needle.empty() || !valid_utf8(needle)) return NeedleStatus::Invalid;
    folded = fold_text(needle, t.lower());
    return folded.size() > kSubMaxNeedle ? NeedleStatus::TooLong : NeedleStatus::Ok;
}

// ---- the device form: shift-and over packed needles (match.hip.h SubLane) ----
// The folded needles are packed first-fit into kSubWords words of 64 bit positions (a needle never straddles a word).  m[b][w]: bit
// p set when the needle byte at position p of word w equals b; start: the first position of every needle; any: the end positions
// of the any-field needles.  where[i] = word | end bit << 8 of needle i.
struct NeedlePack {
    std::vector<uint64_t> m = std::vector<uint64_t>(256 * kSubWords, 0);
    uint64_t start[kSubWords] = {}, any[kSubWords] = {};
    std::vector<uint32_t> where;
};
// false: the needles do not fit (more than 64 * kSubWords bytes in all, or no word has room left for one of them)
inline bool pack_needles(const std::vector<std::string> &folded, const std::vector<uint8_t> &any_field, NeedlePack &out)
{
    uint32_t used[kSubWords] = {};
    for (size_t i = 0; i < folded.size(); ++i) {
        const uint32_t n = (uint32_t)folded[i].size();
        uint32_t w = 0;
        while (w < kSubWords && used[w] + n > 64u) ++w;
        if (n == 0 || w == kSubWords) return false;
        const uint32_t p0 = used[w];
        for (uint32_t k = 0; k < n; ++k) out.m[(size_t)(unsigned char)folded[i][k] * kSubWords + w] |= 1ull << (p0 + k);
        out.start[w] |= 1ull << p0;
        if (any_field[i]) out.any[w] |= 1ull << (p0 + n - 1);
        out.where.push_back(w | (p0 + n - 1) << 8);
        used[w] += n;
    }
    return true;
}

}  // namespace bsh
