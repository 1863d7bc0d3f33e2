// text.hpp — UTF-8 decoding, Unicode white space / simple lower-casing and the
// whitespace+lowercase tokenizer, byte-for-byte as Go's standard library behaves
// for the reference's BasicWhitespaceLowerTokenizer = strings.Fields(strings.ToLower(v))
// (tokenizer.go:141-143) and its zero-alloc twin forEachWord + appendFoldedWord
// (row_matcher.go:142-202); and the separator family it belongs to,
// strings.FieldsFunc(lower ? strings.ToLower(v) : v, isSep) (Tokenizer, for_each_token).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>

namespace bsh {

constexpr uint32_t kRuneError = 0xFFFD;

// utf8.DecodeRuneInString: returns the rune and its width; any invalid or
// truncated sequence (incl. surrogates, overlongs, > U+10FFFF) is (U+FFFD, 1).
inline uint32_t decode_rune(const unsigned char *p, size_t n, size_t &width)
{
    width = 1;
    const unsigned c0 = p[0];
    if (c0 < 0x80) return c0;
    if (c0 < 0xC2) return kRuneError;
    if (c0 < 0xE0) {
        if (n < 2 || (p[1] & 0xC0) != 0x80) return kRuneError;
        width = 2;
        return ((c0 & 0x1F) << 6) | (p[1] & 0x3F);
    }
    if (c0 < 0xF0) {
        if (n < 3) return kRuneError;
        const unsigned lo = c0 == 0xE0 ? 0xA0 : 0x80, hi = c0 == 0xED ? 0x9F : 0xBF;
        if (p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80) return kRuneError;
        width = 3;
        return ((c0 & 0x0F) << 12) | ((p[1] & 0x3F) << 6) | (p[2] & 0x3F);
    }
    if (c0 < 0xF5) {
        if (n < 4) return kRuneError;
        const unsigned lo = c0 == 0xF0 ? 0x90 : 0x80, hi = c0 == 0xF4 ? 0x8F : 0xBF;
        if (p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80 || (p[3] & 0xC0) != 0x80) return kRuneError;
        width = 4;
        return ((c0 & 0x07) << 18) | ((p[1] & 0x3F) << 12) | ((p[2] & 0x3F) << 6) | (p[3] & 0x3F);
    }
    return kRuneError;
}

// utf8.AppendRune (invalid runes and surrogates encode as U+FFFD)
inline void append_rune(std::string &dst, uint32_t r)
{
    if (r > 0x10FFFF || (r >= 0xD800 && r <= 0xDFFF)) r = kRuneError;
    if (r < 0x80) {
        dst.push_back((char)r);
    } else if (r < 0x800) {
        dst.push_back((char)(0xC0 | (r >> 6)));
        dst.push_back((char)(0x80 | (r & 0x3F)));
    } else if (r < 0x10000) {
        dst.push_back((char)(0xE0 | (r >> 12)));
        dst.push_back((char)(0x80 | ((r >> 6) & 0x3F)));
        dst.push_back((char)(0x80 | (r & 0x3F)));
    } else {
        dst.push_back((char)(0xF0 | (r >> 18)));
        dst.push_back((char)(0x80 | ((r >> 12) & 0x3F)));
        dst.push_back((char)(0x80 | ((r >> 6) & 0x3F)));
        dst.push_back((char)(0x80 | (r & 0x3F)));
    }
}

inline bool ascii_space(unsigned char c)  // row_matcher.go:179-181
{
    return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r';
}

// unicode.IsSpace
inline bool is_space(uint32_t r)
{
    if (r < 0x80) return ascii_space((unsigned char)r);
    return r == 0x85 || r == 0xA0 || r == 0x1680 || (r >= 0x2000 && r <= 0x200A) || r == 0x2028 || r == 0x2029 ||
           r == 0x202F || r == 0x205F || r == 0x3000;
}

struct LowerPair { uint32_t from, to; };
inline const LowerPair kLowerTable[] = {
#include "unicode_lower.inc"
};

// Code points this build's tables know nothing about (unassigned in the Unicode version they were generated from): a
// newer Unicode may have made them cased letters.  The device walker never folds them itself — it hands the row to the
// host, whose own unicode.ToLower then decides (a Go host: its toolchain's tables; this mirror: identity).
struct RuneRange { uint32_t from, to; };
inline const RuneRange kUnknownRanges[] = {
#include "unicode_unknown.inc"
};
inline bool is_unknown_rune(uint32_t r)
{
    size_t lo = 0, hi = sizeof(kUnknownRanges) / sizeof(kUnknownRanges[0]);
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (kUnknownRanges[mid].to < r) lo = mid + 1; else hi = mid;
    }
    return lo < sizeof(kUnknownRanges) / sizeof(kUnknownRanges[0]) && kUnknownRanges[lo].from <= r;
}

// unicode.ToLower: simple case mapping (one rune -> one rune)
inline uint32_t to_lower(uint32_t r)
{
    if (r < 0x80) return (r >= 'A' && r <= 'Z') ? r + 32 : r;
    size_t lo = 0, hi = sizeof(kLowerTable) / sizeof(kLowerTable[0]);
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (kLowerTable[mid].from < r) lo = mid + 1; else hi = mid;
    }
    if (lo < sizeof(kLowerTable) / sizeof(kLowerTable[0]) && kLowerTable[lo].from == r) return kLowerTable[lo].to;
    return r;
}

// forEachWord (row_matcher.go:142-177): fn(word) for each maximal run of non-space runes.
template <class F>
inline void for_each_word(std::string_view text, F &&fn)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(text.data());
    const size_t n = text.size();
    size_t i = 0;
    while (i < n) {
        size_t w;
        const uint32_t r = decode_rune(p + i, n - i, w);
        if (is_space(r)) { i += w; continue; }
        const size_t start = i;
        while (i < n) {
            const uint32_t r2 = decode_rune(p + i, n - i, w);
            if (is_space(r2)) break;
            i += w;
        }
        if (!fn(text.substr(start, i - start))) return;
    }
}

// appendFoldedWord (row_matcher.go:187-202): dst += strings.ToLower(word)
inline void append_folded_word(std::string &dst, std::string_view word)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(word.data());
    const size_t n = word.size();
    for (size_t i = 0; i < n;) {
        const unsigned char c = p[i];
        if (c < 0x80) {
            dst.push_back((char)((c >= 'A' && c <= 'Z') ? c + 32 : c));
            ++i;
            continue;
        }
        size_t w;
        const uint32_t r = decode_rune(p + i, n - i, w);
        i += w;
        append_rune(dst, to_lower(r));
    }
}

// A tokenizer of the separator family (bloomgpu.h bsg_tokenizer): tokens = FieldsFunc(lower ? ToLower(text) : text, isSep),
// isSep(r) = bit r of sep for ASCII r, unicode.IsSpace(r) for r >= 0x80 under kUnicodeSpace.  The default members are
// BasicWhitespaceLowerTokenizer's.
struct Tokenizer {
    static constexpr uint32_t kUnicodeSpace = 1, kLower = 2;      // BSG_TOK_UNICODE_SPACE, BSG_TOK_LOWER
    static constexpr uint64_t kWhiteSpace = (1ull << 9) | (1ull << 10) | (1ull << 11) | (1ull << 12) | (1ull << 13) | (1ull << 32);
    uint64_t sep[2] = {kWhiteSpace, 0};
    uint32_t flags = kUnicodeSpace | kLower;
    uint32_t ngram = 0;                                           // BSG_TOK_NGRAM: 0, or 2..4 = a word's windows of that many runes

    static bool valid_ngram(uint64_t n) { return n == 0 || (n >= 2 && n <= 4); }
    bool is_default() const { return sep[0] == kWhiteSpace && sep[1] == 0 && flags == (kUnicodeSpace | kLower) && ngram == 0; }
    bool lower() const { return (flags & kLower) != 0; }
    // the rune AFTER lowering
    bool is_sep(uint32_t r) const { return r < 0x80 ? ((sep[r >> 6] >> (r & 63)) & 1) != 0 : ((flags & kUnicodeSpace) != 0 && is_space(r)); }
    bool operator==(const Tokenizer &o) const { return sep[0] == o.sep[0] && sep[1] == o.sep[1] && flags == o.flags && ngram == o.ngram; }
};

// grams(w, n) of bloomgpu.h: fn(w) if w has at most n runes, else fn(window) for every n consecutive runes of w.  Runes as Go's
// `range` decodes them: an invalid byte is one rune of width 1.  false: fn asked to stop.
template <class F>
inline bool for_each_gram(std::string_view w, uint32_t n, F &&fn)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(w.data());
    size_t start[5];                       // byte offsets of the last n + 1 rune starts, as a ring
    size_t runes = 0;
    for (size_t i = 0; i < w.size();) {
        start[runes % (n + 1)] = i;
        ++runes;
        size_t width;
        (void)decode_rune(p + i, w.size() - i, width);
        i += width;
        if (runes >= n) {
            const size_t from = start[(runes - n) % (n + 1)];
            if (!fn(w.substr(from, i - from))) return false;
        }
    }
    if (runes < n && runes > 0) return fn(w);
    return true;
}

// fn(word) for each word of `text` under t's separators and flags (the width aside), the word's bytes as they are after lowering
// (buf is scratch).  The default tokenizer takes the forEachWord + appendFoldedWord path above.  strings.ToLower turns an
// invalid byte into U+FFFD; without lowering FieldsFunc keeps the raw byte inside its word (it decodes it as U+FFFD, which is
// no separator).
template <class F>
inline void for_each_spec_word(std::string_view text, const Tokenizer &t, std::string &buf, F &&fn)
{
    if (t.sep[0] == Tokenizer::kWhiteSpace && t.sep[1] == 0 && t.flags == (Tokenizer::kUnicodeSpace | Tokenizer::kLower)) {
        for_each_word(text, [&](std::string_view word) {
            buf.clear();
            append_folded_word(buf, word);
            return fn(std::string_view(buf));
        });
        return;
    }
    const unsigned char *p = reinterpret_cast<const unsigned char *>(text.data());
    const size_t n = text.size();
    buf.clear();
    for (size_t i = 0; i < n;) {
        size_t w;
        uint32_t r = decode_rune(p + i, n - i, w);
        if (t.lower()) r = to_lower(r);
        if (t.is_sep(r)) {
            if (!buf.empty()) {
                if (!fn(std::string_view(buf))) return;
                buf.clear();
            }
        } else if (t.lower()) {
            append_rune(buf, r);
        } else {
            buf.append(text.data() + i, w);
        }
        i += w;
    }
    if (!buf.empty()) fn(std::string_view(buf));
}

// ... and with an n-gram width, each of those words cut into its windows (for_each_gram).  The one site the host walker,
// EntrySets, RowMatcher, bsh_tokenize_with and the fallback rows tokenize through.
template <class F>
inline void for_each_token(std::string_view text, const Tokenizer &t, std::string &buf, F &&fn)
{
    if (t.ngram == 0) { for_each_spec_word(text, t, buf, fn); return; }
    for_each_spec_word(text, t, buf, [&](std::string_view word) { return for_each_gram(word, t.ngram, fn); });
}

}  // namespace bsh
