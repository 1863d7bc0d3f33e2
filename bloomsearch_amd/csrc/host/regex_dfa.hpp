// regex_dfa.hpp — a stated subset of Go / RE2 regexp syntax compiled to a byte DFA, for the device row matcher's FieldRegex
// conditions (row_matcher.go:440-573) and its host runner.
//
// Within the subset the answers are exactly Go regexp's MatchString answers; anything outside it — syntax errors included, the
// caller's own engine decides validity — is refused with a message naming the construct.
//   Supported: literals (any rune); escapes \\ \. \* ... (any ASCII punctuation), \t \n \r \f \v \a, \xHH, \x{H...};
//   . ([^\n], every rune under (?s)); bracket classes with ranges, negation, escapes, Perl classes and ASCII POSIX classes
//   ([[:alpha:]], [[:^alpha:]]); \d \D \s \S \w \W with RE2's ASCII definitions (\s = [\t\n\f\r ], no \v); ^ and \A (start
//   of text), $ and \z (end of text only); capturing, non-capturing and named groups; alternation with empty alternatives;
//   * + ? {n} {n,} {n,m}, greedy or lazy, counts <= 1000; flags i, s, U — leading, inline (to the end of the group) or
//   scoped (?i:...).  (?i) folds along unicode.SimpleFold orbits and is supported only over ASCII runes: a letter x is
//   {x, X}, except k = {k, K, U+212A} and s = {s, S, U+017F}; a negated class is folded first and then negated.
//   Refused: \p \P, \b \B, (?m), \C, \Q..\E, back references / octal, (?i) over a non-ASCII rune, malformed syntax, and any
//   pattern whose NFA or DFA grows past kMaxNfaNodes / kMaxDfaStates (subset construction stops AT the cap).
//
// Construction: runes -> UTF-8 byte sequences -> Thompson NFA over bytes (the text anchors are assertions checked at text
// start and end) -> subset construction (capped) -> Moore minimisation -> byte equivalence classes.  Acceptance is sticky
// (the reference asks MatchString: any match anywhere), so every accepting state is absorbing and all of them are one state.
// Transition entries carry the target's flags: kAccept (the text matches whatever follows), kDead (no continuation can
// match), kAcceptAtEnd (the text matches if it ends here).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace bsh_rx {

constexpr uint32_t kMaxDfaStates = 1024;      // before minimisation; also bounds the work per pattern
constexpr uint32_t kMaxNfaNodes = 1u << 16;
constexpr int kMaxRepeat = 1000;              // RE2's limit on {n,m}
constexpr uint16_t kAccept = 0x8000, kDead = 0x4000, kAcceptAtEnd = 0x2000, kStateMask = 0x1FFF;

struct Dfa {
    uint32_t n_states = 0, n_classes = 0;
    uint8_t cls[256] = {};
    std::vector<uint16_t> trans;              // [state * n_classes + class] = target state | the target's flags
    uint16_t start = 0;                       // start state | its flags
};

using Ranges = std::vector<std::pair<uint32_t, uint32_t>>;   // rune ranges, sorted and merged by clean()

inline void clean(Ranges &r)
{
    std::sort(r.begin(), r.end());
    Ranges o;
    for (auto &x : r) {
        if (!o.empty() && x.first <= o.back().second + 1) o.back().second = std::max(o.back().second, x.second);
        else o.push_back(x);
    }
    r.swap(o);
}
inline Ranges negate(Ranges r)
{
    clean(r);
    Ranges o;
    uint32_t next = 0;
    for (auto &x : r) {
        if (x.first > next) o.push_back({next, x.first - 1});
        next = x.second + 1;
    }
    if (next <= 0x10FFFF) o.push_back({next, 0x10FFFF});
    return o;
}

namespace detail {

struct Node {
    enum Kind : uint8_t { Empty, Class, Cat, Alt, Rep, Bol, Eol } k = Empty;
    Ranges cls;
    std::vector<int> kids;
    int min = 0, max = 0;                     // Rep: max -1 = unbounded
};

struct Flags { bool i = false, s = false; };

inline bool is_alnum(uint32_t c) { return (c - '0' < 10u) || ((c | 0x20u) - 'a' < 26u); }

class Parser {
public:
    explicit Parser(std::string_view p) : s_(p) {}
    std::vector<Node> pool;
    std::string err;

    int parse()
    {
        Flags f;
        const int root = alt(f, 0);
        if (root < 0) return -1;
        if (i_ < s_.size()) return fail("unexpected )");
        return root;
    }

private:
    std::string_view s_;
    size_t i_ = 0;

    int fail(const std::string &m) { if (err.empty()) err = m; return -1; }
    int add(Node n) { pool.push_back(std::move(n)); return (int)pool.size() - 1; }
    bool eof() const { return i_ >= s_.size(); }
    uint32_t peek() const { return (uint8_t)s_[i_]; }

    // one rune of the pattern (Go rejects invalid UTF-8 in a pattern)
    bool rune(uint32_t &r)
    {
        const uint8_t *p = (const uint8_t *)s_.data() + i_;
        const size_t n = s_.size() - i_;
        const uint8_t b = p[0];
        if (b < 0x80) { r = b; i_ += 1; return true; }
        uint32_t need, lo = 0x80, hi = 0xBF;
        if (b >= 0xC2 && b <= 0xDF) { need = 1; r = b & 0x1F; }
        else if (b >= 0xE0 && b <= 0xEF) { need = 2; r = b & 0x0F; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { need = 3; r = b & 0x07; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        else return fail("invalid UTF-8 in pattern"), false;
        if (n < need + 1) return fail("invalid UTF-8 in pattern"), false;
        for (uint32_t k = 1; k <= need; ++k) {
            const uint8_t c = p[k];
            if (c < (k == 1 ? lo : 0x80) || c > (k == 1 ? hi : 0xBF)) return fail("invalid UTF-8 in pattern"), false;
            r = (r << 6) | (c & 0x3F);
        }
        i_ += need + 1;
        return true;
    }

    // ASCII simple-fold orbit; false (refused) for a non-ASCII rune under (?i)
    bool fold_range(Ranges &out, uint32_t lo, uint32_t hi)
    {
        if (hi >= 0x80) return fail("(?i) over a non-ASCII rune"), false;
        for (uint32_t c = lo; c <= hi; ++c) {
            out.push_back({c, c});
            const uint32_t l = c | 0x20u;
            if (l - 'a' < 26u) { out.push_back({l, l}); out.push_back({l - 32, l - 32}); }
            if (l == 'k') out.push_back({0x212A, 0x212A});
            if (l == 's') out.push_back({0x17F, 0x17F});
        }
        return true;
    }
    bool add_range(Ranges &out, uint32_t lo, uint32_t hi, const Flags &f)
    {
        if (!f.i) { out.push_back({lo, hi}); return true; }
        return fold_range(out, lo, hi);
    }
    // a Perl / POSIX group: folded (ASCII) under (?i), then negated if asked (parser.go appendGroup)
    bool add_group(Ranges &out, Ranges g, bool neg, const Flags &f)
    {
        if (f.i) {
            Ranges t;
            for (auto &x : g) if (!fold_range(t, x.first, x.second)) return false;
            g.swap(t);
        }
        if (neg) g = negate(g);
        out.insert(out.end(), g.begin(), g.end());
        return true;
    }

    static bool perl_class(uint32_t c, Ranges &g, bool &neg)
    {
        neg = c == 'D' || c == 'S' || c == 'W';
        switch (c | 0x20u) {
        case 'd': g = {{'0', '9'}}; return true;
        case 's': g = {{'\t', '\n'}, {'\f', '\r'}, {' ', ' '}}; return true;
        case 'w': g = {{'0', '9'}, {'A', 'Z'}, {'_', '_'}, {'a', 'z'}}; return true;
        default: return false;
        }
    }
    static bool posix_class(std::string_view n, Ranges &g)
    {
        static const std::map<std::string_view, Ranges> t = {
            {"alnum", {{'0', '9'}, {'A', 'Z'}, {'a', 'z'}}}, {"alpha", {{'A', 'Z'}, {'a', 'z'}}}, {"ascii", {{0, 0x7F}}},
            {"blank", {{'\t', '\t'}, {' ', ' '}}}, {"cntrl", {{0, 0x1F}, {0x7F, 0x7F}}}, {"digit", {{'0', '9'}}},
            {"graph", {{'!', '~'}}}, {"lower", {{'a', 'z'}}}, {"print", {{' ', '~'}}},
            {"punct", {{'!', '/'}, {':', '@'}, {'[', '`'}, {'{', '~'}}}, {"space", {{'\t', '\r'}, {' ', ' '}}},
            {"upper", {{'A', 'Z'}}}, {"word", {{'0', '9'}, {'A', 'Z'}, {'a', 'z'}, {'_', '_'}}},
            {"xdigit", {{'0', '9'}, {'A', 'F'}, {'a', 'f'}}}};
        auto it = t.find(n);
        if (it == t.end()) return false;
        g = it->second;
        return true;
    }

    bool hex_digits(uint32_t &v, size_t n_min, size_t n_max, char stop)
    {
        v = 0;
        size_t n = 0;
        while (!eof() && (stop == 0 ? n < n_max : peek() != (uint32_t)stop)) {
            const uint32_t c = peek(), l = c | 0x20u;
            uint32_t d;
            if (c - '0' < 10u) d = c - '0';
            else if (l - 'a' < 6u) d = l - 'a' + 10;
            else return fail("malformed \\x escape"), false;
            v = v * 16 + d;
            if (v > 0x10FFFF) return fail("\\x escape above U+10FFFF"), false;
            ++i_; ++n;
        }
        if (n < n_min || (stop != 0 && eof())) return fail("malformed \\x escape"), false;
        if (stop != 0) ++i_;
        return true;
    }

    // a single-rune escape after the backslash (parser.go parseEscape, restricted to the subset)
    bool escape_rune(uint32_t &r)
    {
        if (eof()) return fail("trailing backslash"), false;
        const uint32_t c = peek();
        if (c < 0x80 && !is_alnum(c)) { ++i_; r = c; return true; }
        switch (c) {
        case 't': ++i_; r = '\t'; return true;
        case 'n': ++i_; r = '\n'; return true;
        case 'r': ++i_; r = '\r'; return true;
        case 'f': ++i_; r = '\f'; return true;
        case 'v': ++i_; r = '\v'; return true;
        case 'a': ++i_; r = 7; return true;
        case 'x':
            ++i_;
            if (!eof() && peek() == '{') { ++i_; return hex_digits(r, 1, 0, '}'); }
            return hex_digits(r, 2, 2, 0);
        default: {
            std::string m = "escape \\";
            if (c < 0x80) m += (char)c; else m += "<non-ASCII>";
            return fail(m), false;
        }
        }
    }

    int bracket(const Flags &f)
    {
        ++i_;                                                     // '['
        bool neg = false;
        if (!eof() && peek() == '^') { neg = true; ++i_; }
        Ranges cls;
        bool first = true;
        while (first || eof() || peek() != ']') {
            if (eof()) return fail("missing ]");
            first = false;
            if (s_.size() - i_ > 2 && s_[i_] == '[' && s_[i_ + 1] == ':') {
                const size_t e = s_.find(":]", i_ + 2);
                if (e != std::string_view::npos) {
                    std::string_view name = s_.substr(i_ + 2, e - i_ - 2);
                    bool gneg = false;
                    if (!name.empty() && name[0] == '^') { gneg = true; name.remove_prefix(1); }
                    Ranges g;
                    if (!posix_class(name, g)) return fail("unknown POSIX class [:" + std::string(name) + ":]");
                    if (!add_group(cls, g, gneg, f)) return -1;
                    i_ = e + 2;
                    continue;
                }
            }
            if (peek() == '\\' && i_ + 1 < s_.size()) {
                const uint32_t c = (uint8_t)s_[i_ + 1];
                Ranges g;
                bool gneg;
                if (perl_class(c, g, gneg)) {
                    i_ += 2;
                    if (!add_group(cls, g, gneg, f)) return -1;
                    continue;
                }
                if (c == 'p' || c == 'P') return fail("Unicode class \\p / \\P");
            }
            uint32_t lo, hi;
            if (!class_char(lo)) return -1;
            hi = lo;
            if (s_.size() - i_ >= 2 && s_[i_] == '-' && s_[i_ + 1] != ']') {
                ++i_;
                if (!class_char(hi)) return -1;
                if (hi < lo) return fail("invalid class range");
            }
            if (!add_range(cls, lo, hi, f)) return -1;
        }
        ++i_;                                                     // ']'
        clean(cls);
        Node n;
        n.k = Node::Class;
        n.cls = neg ? negate(cls) : cls;
        return add(std::move(n));
    }
    bool class_char(uint32_t &r)
    {
        if (eof()) return fail("missing ]"), false;
        if (peek() == '\\') { ++i_; return escape_rune(r); }
        return rune(r);
    }

    // {n}, {n,}, {n,m}: 1 parsed, 0 not a repeat ('{' is a literal), -1 refused
    int repeat(int &mn, int &mx)
    {
        size_t j = i_ + 1;
        auto num = [&](int &v) -> int {
            const size_t b = j;
            while (j < s_.size() && (uint8_t)s_[j] - '0' < 10u) ++j;
            if (j == b) return 0;
            if (j - b > 1 && s_[b] == '0') return -1;
            if (j - b > 4) return -1;
            v = std::stoi(std::string(s_.substr(b, j - b)));
            return 1;
        };
        int r = num(mn);
        if (r <= 0) return r == 0 && (j >= s_.size() || (uint8_t)s_[j] - '0' >= 10u) ? 0 : fail("malformed repeat");
        if (j < s_.size() && s_[j] == ',') {
            ++j;
            if (j < s_.size() && s_[j] == '}') mx = -1;
            else if ((r = num(mx)) <= 0) return fail("malformed repeat");
        } else {
            mx = mn;
        }
        if (j >= s_.size() || s_[j] != '}') return fail("malformed repeat");
        if (mn > kMaxRepeat || mx > kMaxRepeat || (mx >= 0 && mx < mn)) return fail("invalid repeat count");
        i_ = j + 1;
        return 1;
    }

    int alt(Flags &f, int depth)
    {
        if (depth > 200) return fail("nesting too deep");
        std::vector<int> alts;
        for (;;) {
            const int c = cat(f, depth);
            if (c < 0) return -1;
            alts.push_back(c);
            if (!eof() && peek() == '|') { ++i_; continue; }
            break;
        }
        if (alts.size() == 1) return alts[0];
        Node n;
        n.k = Node::Alt;
        n.kids = alts;
        return add(std::move(n));
    }

    int cat(Flags &f, int depth)
    {
        std::vector<int> items;
        bool can_repeat = false;                                  // the last thing parsed is an atom, not yet repeated
        while (!eof() && peek() != '|' && peek() != ')') {
            const uint32_t c = peek();
            if (c == '*' || c == '+' || c == '?' || (c == '{' && i_ + 1 < s_.size() && (uint8_t)s_[i_ + 1] - '0' < 10u)) {
                int mn = 0, mx = -1;
                if (c == '*') { mn = 0; mx = -1; ++i_; }
                else if (c == '+') { mn = 1; mx = -1; ++i_; }
                else if (c == '?') { mn = 0; mx = 1; ++i_; }
                else {
                    const int r = repeat(mn, mx);
                    if (r < 0) return -1;
                    if (r == 0) goto literal;
                }
                if (!can_repeat) return fail(items.empty() ? "missing argument to repetition operator" : "nested repetition operator");
                if (!eof() && peek() == '?') ++i_;                // lazy: same yes / no answer
                Node n;
                n.k = Node::Rep;
                n.kids = {items.back()};
                n.min = mn; n.max = mx;
                items.back() = add(std::move(n));
                can_repeat = false;
                continue;
            }
            if (c == '(') {
                ++i_;
                Flags g = f;
                if (!eof() && peek() == '?') {
                    ++i_;
                    if (!eof() && (peek() == 'P' || peek() == '<')) {
                        if (peek() == 'P') ++i_;
                        if (eof() || peek() != '<') return fail("unsupported (?P construct");
                        ++i_;
                        const size_t b = i_;
                        while (!eof() && peek() != '>') {
                            const uint32_t k = peek();
                            if (!is_alnum(k) && k != '_') return fail("invalid group name");
                            ++i_;
                        }
                        if (eof() || i_ == b) return fail("invalid group name");
                        ++i_;
                    } else {
                        bool neg = false, any = false, any_after_neg = false;
                        for (;;) {
                            if (eof()) return fail("missing )");
                            const uint32_t k = peek();
                            ++i_;
                            if (k == 'i') { g.i = !neg; any = true; any_after_neg = neg; }
                            else if (k == 's') { g.s = !neg; any = true; any_after_neg = neg; }
                            else if (k == 'U') { any = true; any_after_neg = neg; }
                            else if (k == 'm') return fail("flag (?m)");
                            else if (k == '-') { if (neg) return fail("malformed flags"); neg = true; any_after_neg = false; }
                            else if (k == ')' || k == ':') {
                                if ((!any && (k == ')' || neg)) || (neg && !any_after_neg)) return fail("malformed flags");   // (?:re) is a plain group
                                if (k == ')') { f = g; can_repeat = false; goto next; }
                                break;
                            } else {
                                return fail("unsupported group construct (?" + std::string(1, (char)k));
                            }
                        }
                    }
                }
                {
                    const int inner = alt(g, depth + 1);
                    if (inner < 0) return -1;
                    if (eof() || peek() != ')') return fail("missing )");
                    ++i_;
                    items.push_back(inner);
                    can_repeat = true;
                }
            next:
                continue;
            }
            if (c == '^' || c == '$') {
                ++i_;
                Node n;
                n.k = c == '^' ? Node::Bol : Node::Eol;
                items.push_back(add(std::move(n)));
                can_repeat = true;
                continue;
            }
            if (c == '[') {
                const int b = bracket(f);
                if (b < 0) return -1;
                items.push_back(b);
                can_repeat = true;
                continue;
            }
            if (c == '.') {
                ++i_;
                Node n;
                n.k = Node::Class;
                n.cls = f.s ? Ranges{{0, 0x10FFFF}} : Ranges{{0, '\n' - 1}, {'\n' + 1, 0x10FFFF}};
                items.push_back(add(std::move(n)));
                can_repeat = true;
                continue;
            }
            if (c == '\\' && i_ + 1 < s_.size()) {
                const uint32_t e = (uint8_t)s_[i_ + 1];
                Ranges g;
                bool gneg;
                if (e == 'A' || e == 'z') {
                    i_ += 2;
                    Node n;
                    n.k = e == 'A' ? Node::Bol : Node::Eol;
                    items.push_back(add(std::move(n)));
                    can_repeat = true;
                    continue;
                }
                if (perl_class(e, g, gneg)) {
                    i_ += 2;
                    Node n;
                    n.k = Node::Class;
                    if (!add_group(n.cls, g, gneg, f)) return -1;
                    clean(n.cls);
                    items.push_back(add(std::move(n)));
                    can_repeat = true;
                    continue;
                }
                if (e == 'p' || e == 'P') return fail("Unicode class \\p / \\P");
                if (e == 'b' || e == 'B') return fail("word boundary \\b / \\B");
                if (e == 'C') return fail("\\C");
                if (e == 'Q') return fail("\\Q...\\E");
            }
        literal: {
            uint32_t r;
            if (c == '\\') { ++i_; if (!escape_rune(r)) return -1; }
            else if (!rune(r)) return -1;
            Node n;
            n.k = Node::Class;
            if (!add_range(n.cls, r, r, f)) return -1;
            clean(n.cls);
            items.push_back(add(std::move(n)));
            can_repeat = true;
        }
        }
        if (items.size() == 1) return items[0];
        Node n;
        n.k = items.empty() ? Node::Empty : Node::Cat;
        n.kids = items;
        return add(std::move(n));
    }
};

// ---- Thompson NFA over bytes ----
struct SetHash {
    size_t operator()(const std::vector<int> &v) const
    {
        uint64_t h = 0x9E3779B97F4A7C15ull ^ v.size();
        for (int x : v) h = (h ^ (uint32_t)x) * 0x100000001B3ull;
        return (size_t)(h ^ (h >> 29));
    }
};

struct NState {
    enum Kind : uint8_t { Byte, Split, Eps, Bol, Eol, Match } k;
    uint8_t lo = 0, hi = 0;
    int out = -1, out1 = -1;
};

// UTF-8 byte-range sequences of the rune range [lo, hi] (surrogates excluded): the standard split at encoding-length and
// continuation-byte boundaries
inline void utf8_sequences(uint32_t lo, uint32_t hi, std::vector<std::vector<std::pair<uint8_t, uint8_t>>> &out)
{
    std::vector<std::pair<uint32_t, uint32_t>> todo{{lo, hi}};
    auto enc = [](uint32_t r, uint8_t *b) -> int {
        if (r < 0x80) { b[0] = (uint8_t)r; return 1; }
        if (r < 0x800) { b[0] = 0xC0 | (r >> 6); b[1] = 0x80 | (r & 0x3F); return 2; }
        if (r < 0x10000) { b[0] = 0xE0 | (r >> 12); b[1] = 0x80 | ((r >> 6) & 0x3F); b[2] = 0x80 | (r & 0x3F); return 3; }
        b[0] = 0xF0 | (r >> 18); b[1] = 0x80 | ((r >> 12) & 0x3F); b[2] = 0x80 | ((r >> 6) & 0x3F); b[3] = 0x80 | (r & 0x3F);
        return 4;
    };
    while (!todo.empty()) {
        auto [a, b] = todo.back();
        todo.pop_back();
        if (a > b) continue;
        if (a <= 0xDFFF && b >= 0xD800) {                         // no surrogates
            if (a < 0xD800) todo.push_back({a, 0xD7FF});
            if (b > 0xDFFF) todo.push_back({0xE000, b});
            continue;
        }
        bool split = false;
        for (uint32_t m : {0x7Fu, 0x7FFu, 0xFFFFu})
            if (a <= m && b > m) { todo.push_back({a, m}); todo.push_back({m + 1, b}); split = true; break; }
        if (split) continue;
        if (b < 0x80) { out.push_back({{(uint8_t)a, (uint8_t)b}}); continue; }
        for (int k = 1; k < 4 && !split; ++k) {
            const uint32_t mx = (1u << (6 * k)) - 1;
            if ((a & ~mx) != (b & ~mx)) {
                if ((a & mx) != 0) { todo.push_back({a, a | mx}); todo.push_back({(a | mx) + 1, b}); split = true; }
                else if ((b & mx) != mx) { todo.push_back({a, (b & ~mx) - 1}); todo.push_back({b & ~mx, b}); split = true; }
            }
        }
        if (split) continue;
        uint8_t ea[4], eb[4];
        const int n = enc(a, ea);
        enc(b, eb);
        std::vector<std::pair<uint8_t, uint8_t>> seq;
        for (int k = 0; k < n; ++k) seq.push_back({ea[k], eb[k]});
        out.push_back(seq);
    }
}

class NfaBuilder {
public:
    std::vector<NState> st;
    std::string err;
    const std::vector<Node> &pool;
    explicit NfaBuilder(const std::vector<Node> &p) : pool(p) {}

    int make(NState s)
    {
        if (st.size() >= kMaxNfaNodes) { if (err.empty()) err = "pattern too large (NFA)"; return -1; }
        st.push_back(s);
        return (int)st.size() - 1;
    }
    // compile node n so that it continues at `next`; returns its entry (continuation-passing Thompson construction)
    int build(int n, int next)
    {
        if (next < 0) return -1;
        const Node &x = pool[n];
        switch (x.k) {
        case Node::Empty: return next;
        case Node::Bol: return make({NState::Bol, 0, 0, next, -1});
        case Node::Eol: return make({NState::Eol, 0, 0, next, -1});
        case Node::Class: {
            std::vector<std::vector<std::pair<uint8_t, uint8_t>>> seqs;
            for (auto &r : x.cls) utf8_sequences(r.first, r.second, seqs);
            if (seqs.empty()) return make({NState::Split, 0, 0, -1, -1});   // matches nothing
            int entry = -1;
            for (auto &q : seqs) {
                int cur = next;
                for (int k = (int)q.size() - 1; k >= 0; --k) {
                    cur = make({NState::Byte, q[k].first, q[k].second, cur, -1});
                    if (cur < 0) return -1;
                }
                entry = entry < 0 ? cur : make({NState::Split, 0, 0, cur, entry});
                if (entry < 0) return -1;
            }
            return entry;
        }
        case Node::Cat: {
            int cur = next;
            for (int k = (int)x.kids.size() - 1; k >= 0 && cur >= 0; --k) cur = build(x.kids[k], cur);
            return cur;
        }
        case Node::Alt: {
            int entry = -1;
            for (int k = (int)x.kids.size() - 1; k >= 0; --k) {
                const int b = build(x.kids[k], next);
                if (b < 0) return -1;
                entry = entry < 0 ? b : make({NState::Split, 0, 0, b, entry});
                if (entry < 0) return -1;
            }
            return entry;
        }
        case Node::Rep: {
            int cur;
            if (x.max < 0) {
                const int loop = make({NState::Split, 0, 0, -1, next});
                if (loop < 0) return -1;
                const int body = build(x.kids[0], loop);
                if (body < 0) return -1;
                st[loop].out = body;
                cur = loop;
            } else {
                cur = next;
                for (int k = 0; k < x.max - x.min && cur >= 0; ++k) {
                    const int b = build(x.kids[0], cur);
                    cur = b < 0 ? -1 : make({NState::Split, 0, 0, b, next});
                }
            }
            for (int k = 0; k < x.min && cur >= 0; ++k) cur = build(x.kids[0], cur);
            return cur;
        }
        }
        return -1;
    }
};

}  // namespace detail

// Compile `pattern`; false with `err` naming the construct when it is outside the subset.
inline bool compile(std::string_view pattern, Dfa &out, std::string &err)
{
    using namespace detail;
    Parser p(pattern);
    const int root = p.parse();
    if (root < 0) { err = p.err; return false; }
    NfaBuilder nb(p.pool);
    const int match = nb.make({NState::Match, 0, 0, -1, -1});
    const int body = nb.build(root, match);
    // Unanchored search is a loop that skips any byte in front of the pattern.  Skipping BYTES rather than runes is exact
    // because every text the DFA sees is valid UTF-8 (the host runner feeds an invalid byte as the 3 bytes of U+FFFD; the
    // device hands rows with invalid UTF-8 back to the host): a match can never begin on a continuation byte, since every
    // byte sequence the pattern consumes starts with the lead byte of a rune, and the empty-width assertions only hold at
    // the very start or end of the text.
    const int skip = nb.make({NState::Byte, 0x00, 0xFF, -1, -1});
    const int start = body < 0 || skip < 0 ? -1 : nb.make({NState::Split, 0, 0, body, skip});
    if (start < 0) { err = nb.err.empty() ? "pattern too large (NFA)" : nb.err; return false; }
    nb.st[skip].out = start;
    const std::vector<NState> &S = nb.st;

    // byte classes of the NFA: bytes no Byte state tells apart
    bool cut[257] = {};
    for (auto &s : S) if (s.k == NState::Byte) { cut[s.lo] = true; cut[s.hi + 1] = true; }
    std::vector<uint8_t> rep;
    for (int b = 0; b < 256; ++b) if (b == 0 || cut[b]) rep.push_back((uint8_t)b);

    std::vector<uint32_t> mark(S.size(), 0);
    uint32_t stamp = 0;
    std::vector<int> stack;
    // the Byte / Match / Eol states reachable through empty moves (Bol only at the text start, Eol followed only at its end)
    auto closure = [&](const std::vector<int> &seeds, bool at_start, bool at_end, std::vector<int> &set) {
        ++stamp;
        set.clear();
        stack.assign(seeds.begin(), seeds.end());
        while (!stack.empty()) {
            const int x = stack.back();
            stack.pop_back();
            if (x < 0 || mark[x] == stamp) continue;
            mark[x] = stamp;
            const NState &s = S[x];
            switch (s.k) {
            case NState::Byte: case NState::Match: set.push_back(x); break;
            case NState::Split: stack.push_back(s.out1); stack.push_back(s.out); break;
            case NState::Eps: stack.push_back(s.out); break;
            case NState::Bol: if (at_start) stack.push_back(s.out); break;
            case NState::Eol: if (at_end) stack.push_back(s.out); else set.push_back(x); break;
            }
        }
        std::sort(set.begin(), set.end());
    };
    auto has_match = [&](const std::vector<int> &set) {
        for (int x : set) if (S[x].k == NState::Match) return true;
        return false;
    };

    std::vector<std::vector<int>> sets;
    std::vector<uint8_t> acc, acc_end;
    std::vector<std::vector<uint32_t>> tr;                        // [state][rep]
    std::unordered_map<std::vector<int>, uint32_t, SetHash> index;
    std::vector<int> set, seeds;
    closure({start}, true, false, set);
    sets.push_back(set);                                          // (the start state is never a transition's target: not indexed)
    acc.push_back(has_match(set));
    closure({start}, true, true, set);
    acc_end.push_back(has_match(set));
    for (size_t q = 0; q < sets.size(); ++q) {
        tr.emplace_back(rep.size(), (uint32_t)q);
        if (acc[q]) continue;                                     // sticky: an accepting state is absorbing
        for (size_t ri = 0; ri < rep.size(); ++ri) {
            const uint8_t b = rep[ri];
            seeds.clear();
            for (int x : sets[q]) if (S[x].k == NState::Byte && S[x].lo <= b && b <= S[x].hi) seeds.push_back(S[x].out);
            closure(seeds, false, false, set);
            auto it = index.find(set);
            uint32_t t;
            if (it != index.end()) {
                t = it->second;
            } else {
                if (sets.size() >= kMaxDfaStates) { err = "DFA exceeds " + std::to_string(kMaxDfaStates) + " states"; return false; }
                t = (uint32_t)sets.size();
                index.emplace(set, t);
                sets.push_back(set);
                acc.push_back(has_match(set));
                seeds.clear();
                for (int x : set) if (S[x].k == NState::Eol) seeds.push_back(S[x].out);
                std::vector<int> e;
                closure(seeds, false, true, e);
                acc_end.push_back(acc.back() || has_match(e));
            }
            tr[q][ri] = t;
        }
    }
    const uint32_t n = (uint32_t)sets.size(), nr = (uint32_t)rep.size();

    // dead: no accepting (or accept-at-end) state reachable
    std::vector<std::vector<uint32_t>> rev(n);
    for (uint32_t q = 0; q < n; ++q) for (uint32_t t : tr[q]) rev[t].push_back(q);
    std::vector<uint8_t> live(n, 0);
    std::vector<uint32_t> work;
    for (uint32_t q = 0; q < n; ++q) if (acc[q] || acc_end[q]) { live[q] = 1; work.push_back(q); }
    while (!work.empty()) {
        const uint32_t q = work.back();
        work.pop_back();
        for (uint32_t p2 : rev[q]) if (!live[p2]) { live[p2] = 1; work.push_back(p2); }
    }

    // Moore minimisation
    std::vector<uint32_t> blk(n);
    for (uint32_t q = 0; q < n; ++q) blk[q] = acc[q] ? 0 : !live[q] ? 1 : acc_end[q] ? 2 : 3;
    uint32_t n_blk = 0;
    for (;;) {
        std::map<std::vector<uint32_t>, uint32_t> sig;
        std::vector<uint32_t> nb2(n);
        std::vector<uint32_t> key(nr + 1);
        for (uint32_t q = 0; q < n; ++q) {
            key[0] = blk[q];
            for (uint32_t r = 0; r < nr; ++r) key[r + 1] = blk[tr[q][r]];
            auto it = sig.emplace(key, (uint32_t)sig.size()).first;
            nb2[q] = it->second;
        }
        const uint32_t cnt = (uint32_t)sig.size();
        blk.swap(nb2);
        if (cnt == n_blk) break;
        n_blk = cnt;
    }
    // renumber: the start state's block is state 0
    std::vector<uint32_t> id(n_blk, UINT32_MAX), repr;
    id[blk[0]] = 0;
    repr.push_back(0);
    for (uint32_t q = 0; q < n; ++q)
        if (id[blk[q]] == UINT32_MAX) { id[blk[q]] = (uint32_t)repr.size(); repr.push_back(q); }
    const uint32_t m = (uint32_t)repr.size();
    if (m > kStateMask) { err = "DFA too large"; return false; }
    auto flags = [&](uint32_t q) -> uint16_t {
        return (uint16_t)((acc[q] ? kAccept | kAcceptAtEnd : 0) | (!live[q] ? kDead : 0) | (acc_end[q] ? kAcceptAtEnd : 0));
    };
    // byte classes of the minimal DFA: NFA classes whose columns agree
    std::vector<uint32_t> col_cls(nr);
    std::map<std::vector<uint32_t>, uint32_t> cols;
    for (uint32_t r = 0; r < nr; ++r) {
        std::vector<uint32_t> c(m);
        for (uint32_t s = 0; s < m; ++s) c[s] = id[blk[tr[repr[s]][r]]];
        col_cls[r] = cols.emplace(c, (uint32_t)cols.size()).first->second;
    }
    out.n_states = m;
    out.n_classes = (uint32_t)cols.size();
    for (int b = 0, r = -1; b < 256; ++b) {
        if (r + 1 < (int)nr && rep[r + 1] == b) ++r;
        out.cls[b] = (uint8_t)col_cls[r];
    }
    out.trans.assign((size_t)m * out.n_classes, 0);
    for (uint32_t s = 0; s < m; ++s)
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t t = tr[repr[s]][r];
            out.trans[(size_t)s * out.n_classes + col_cls[r]] = (uint16_t)(id[blk[t]] | flags(t));
        }
    out.start = flags(0);
    return true;
}

// MatchString on text as Go sees it: an invalid byte is U+FFFD of width 1 (utf8.DecodeRune), fed as its 3 UTF-8 bytes.
inline bool run(const Dfa &d, const uint8_t *t, size_t n)
{
    uint16_t v = d.start;
    auto feed = [&](uint8_t b) { v = d.trans[(size_t)(v & kStateMask) * d.n_classes + d.cls[b]]; };
    for (size_t i = 0; i < n && !(v & (kAccept | kDead));) {
        const uint8_t b = t[i];
        uint32_t need = 0, lo = 0x80, hi = 0xBF;
        if (b < 0x80) { feed(b); ++i; continue; }
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b >= 0xE0 && b <= 0xEF) { need = 2; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { need = 3; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        bool ok = need > 0;
        for (uint32_t k = 1; ok && k <= need; ++k) {
            if (i + k >= n) { ok = false; break; }
            const uint8_t c = t[i + k];
            if (c < (k == 1 ? lo : 0x80u) || c > (k == 1 ? hi : 0xBFu)) ok = false;
        }
        if (!ok) { feed(0xEF); feed(0xBF); feed(0xBD); ++i; continue; }
        for (uint32_t k = 0; k <= need; ++k) feed(t[i + k]);
        i += need + 1;
    }
    return (v & kAccept) || ((v & kAcceptAtEnd) && !(v & kDead));
}

}  // namespace bsh_rx
