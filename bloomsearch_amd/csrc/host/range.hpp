// range.hpp — numeric range conditions: "some number leaf whose path equals the field has a value inside the interval".
//   * DecimalLiteral / literal_inside: a JSON number literal normalised to (sign, digit string without leading or trailing zeros,
//     position of the decimal point) and compared with int64 bounds digit by digit.  Exact for EVERY literal the JSON grammar allows —
//     any number of digits, fractions, exponents of any size — and free of floating point.
//   * RangeExpression: CONDITION | AND | OR over {"Field", "Lo"?, "Hi"?, "LoOpen"?, "HiOpen"?} (int64 values, an absent or null bound
//     = unbounded), shaped as the regex and substring trees.
//   * range_guard: the tree with every condition replaced by Field(field) — a leaf's own path is a field-existence entry of the
//     filters — under the substring guard's rules: the nil condition (always true) is dropped from an And and KEPT in an Or.
//   * emit_range_program: the tree as the tail of a device row-matcher program (bsg_match_rows_range): a condition's entry 2c + 1 is
//     lo, hi (little-endian int64) and the BSG_RANGE_* flag byte.
//   * RangeRowMatcher: the exact test per row (the matcher of fallback rows; the device tests compare with it).  Strings, true, false
//     and null never hold; a leaf without a path is no candidate (the walker does not emit it); an empty field never holds.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <string_view>
#include <vector>

#include "expression.hpp"
#include "walker.hpp"

namespace bsh {

// value = (neg ? -1 : 1) * 0.d1 d2 .. dn * 10^point, d1 != 0 and dn != 0; digits empty = zero
struct DecimalLiteral {
    bool neg = false;
    std::string digits;
    int64_t point = 0;
};

// -?digits[.digits][(e|E)[+-]digits]: what the JSON scanner accepted as a number.  false for anything else.
inline bool parse_decimal_literal(std::string_view s, DecimalLiteral &out)
{
    out = DecimalLiteral{};
    size_t i = 0;
    if (i < s.size() && s[i] == '-') { out.neg = true; ++i; }
    const size_t int0 = i;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') out.digits.push_back(s[i++]);
    if (i == int0) return false;
    out.point = (int64_t)out.digits.size();
    if (i < s.size() && s[i] == '.') {
        const size_t f0 = ++i;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9') out.digits.push_back(s[i++]);
        if (i == f0) return false;
    }
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
        const size_t e0 = i;
        int64_t e = 0;
        constexpr int64_t kCap = int64_t(1) << 40;     // beyond any digit count a row can hold: the order of magnitude alone decides
        while (i < s.size() && s[i] >= '0' && s[i] <= '9') { if (e < kCap) e = e * 10 + (s[i] - '0'); ++i; }
        if (i == e0) return false;
        out.point += eneg ? -e : e;
    }
    if (i != s.size()) return false;
    size_t lead = 0;
    while (lead < out.digits.size() && out.digits[lead] == '0') ++lead;
    out.digits.erase(0, lead);
    out.point -= (int64_t)lead;
    while (!out.digits.empty() && out.digits.back() == '0') out.digits.pop_back();
    if (out.digits.empty()) { out.point = 0; out.neg = false; }   // -0 and -0.0 are 0
    return true;
}

// sign of (|v| - k)
inline int compare_magnitude(const DecimalLiteral &v, uint64_t k)
{
    std::string kd = k ? std::to_string(k) : std::string();
    const int64_t kpoint = (int64_t)kd.size();
    while (!kd.empty() && kd.back() == '0') kd.pop_back();
    if (v.digits.empty() || kd.empty()) return v.digits.empty() ? (kd.empty() ? 0 : -1) : 1;
    if (v.point != kpoint) return v.point > kpoint ? 1 : -1;       // both lead with a non-zero digit: the point's position orders them
    const int c = v.digits.compare(kd);                             // neither ends in a zero: a proper prefix is the smaller one
    return c < 0 ? -1 : c > 0 ? 1 : 0;
}

// sign of (v - b)
inline int compare_literal(const DecimalLiteral &v, int64_t b)
{
    const bool vneg = v.neg && !v.digits.empty();
    if (vneg != (b < 0)) return vneg ? -1 : 1;
    const uint64_t k = b < 0 ? uint64_t(0) - (uint64_t)b : (uint64_t)b;
    return vneg ? -compare_magnitude(v, k) : compare_magnitude(v, k);
}

struct RangeBounds {
    bool has_lo = false, has_hi = false, lo_open = false, hi_open = false;
    int64_t lo = 0, hi = 0;
    uint8_t flags() const
    {
        return (uint8_t)((has_lo ? 0u : BSG_RANGE_NO_LO) | (has_hi ? 0u : BSG_RANGE_NO_HI) | (lo_open ? BSG_RANGE_LO_OPEN : 0u) | (hi_open ? BSG_RANGE_HI_OPEN : 0u));
    }
};

inline bool literal_inside(const DecimalLiteral &v, const RangeBounds &b)
{
    if (b.has_lo) { const int c = compare_literal(v, b.lo); if (b.lo_open ? c <= 0 : c < 0) return false; }
    if (b.has_hi) { const int c = compare_literal(v, b.hi); if (b.hi_open ? c >= 0 : c > 0) return false; }
    return true;
}

// ---- the query tree ----
struct RangeExpression {
    RegexType type = RegexType::Unknown;       // CONDITION | AND | OR, as the regex tree
    bool has_condition = false;
    std::string field;
    RangeBounds bounds;
    std::vector<RangeExpression> children;
};
inline RangeExpression FieldRange(std::string field, RangeBounds b)
{
    RangeExpression e; e.type = RegexType::Condition; e.has_condition = true; e.field = std::move(field); e.bounds = b;
    return e;
}
// an int64 as a JSON number without fraction or exponent
inline bool int64_from_json(const JNode &n, int64_t &out)
{
    if (n.type != JType::Number || n.text.empty()) return false;
    const std::string &t = n.text;
    const size_t d0 = t[0] == '-' ? 1 : 0;
    if (d0 == t.size() || t.size() - d0 > 19) return false;
    for (size_t i = d0; i < t.size(); ++i) if (t[i] < '0' || t[i] > '9') return false;
    uint64_t mag = 0;
    for (size_t i = d0; i < t.size(); ++i) mag = mag * 10 + (uint64_t)(t[i] - '0');   // <= 19 digits: no wrap
    if (mag > (uint64_t(1) << 63) - (d0 ? 0 : 1)) return false;
    out = d0 ? (int64_t)(uint64_t(0) - mag) : (int64_t)mag;
    return true;
}
inline bool range_expression_from_json(const JNode &n, RangeExpression &out)
{
    if (n.type != JType::Object) return false;
    const JNode *t = n.get("ExpressionType");
    const std::string ts = (t && t->type == JType::String) ? t->text : "";
    out.type = ts == "CONDITION" ? RegexType::Condition : ts == "AND" ? RegexType::And : ts == "OR" ? RegexType::Or : RegexType::Unknown;
    const JNode *c = n.get("Condition");
    out.has_condition = c && c->type == JType::Object;
    if (out.has_condition) {
        const JNode *f = c->get("Field"), *lo = c->get("Lo"), *hi = c->get("Hi"), *lo_open = c->get("LoOpen"), *hi_open = c->get("HiOpen");
        out.field = (f && f->type == JType::String) ? f->text : "";
        out.bounds = RangeBounds{};
        out.bounds.has_lo = lo && lo->type != JType::Null;
        out.bounds.has_hi = hi && hi->type != JType::Null;
        if (out.bounds.has_lo && !int64_from_json(*lo, out.bounds.lo)) return false;
        if (out.bounds.has_hi && !int64_from_json(*hi, out.bounds.hi)) return false;
        out.bounds.lo_open = lo_open && lo_open->type == JType::True;
        out.bounds.hi_open = hi_open && hi_open->type == JType::True;
    }
    const JNode *kids = n.get("Children");
    if (kids && kids->type == JType::Array) {
        out.children.resize(kids->items.size());
        for (size_t i = 0; i < kids->items.size(); ++i)
            if (!range_expression_from_json(kids->items[i], out.children[i])) return false;
    }
    return true;
}

// The guard of a (sub)tree; false = the nil expression (always true).
inline bool range_to_bloom_expression(const RangeExpression &e, BloomExpression &out)
{
    switch (e.type) {
    case RegexType::Condition:
        if (!e.has_condition) return false;
        out = Field(e.field);
        return true;
    case RegexType::And:
    case RegexType::Or: {
        const bool is_and = e.type == RegexType::And;
        out = BloomExpression{};
        out.type = is_and ? ExprType::And : ExprType::Or;
        for (const RangeExpression &c : e.children) {
            BloomExpression child;
            if (range_to_bloom_expression(c, child)) out.children.push_back(std::move(child));
            else if (!is_and) {                // the nil condition stays in its place: the Or is true
                child = BloomExpression{};
                child.type = ExprType::Condition;
                child.has_condition = false;
                out.children.push_back(std::move(child));
            }
        }
        if (is_and && out.children.empty() && !e.children.empty()) return false;   // every child was always true
        return true;
    }
    default:
        return false;                          // an unknown node never matches a row: no guard is needed to stay a superset
    }
}
inline bool range_guard(const RangeExpression *range, BloomExpression &out)
{
    return range && range_to_bloom_expression(*range, out);
}

// lo, hi (little-endian) and the flag byte: entry 2c + 1 of a BSG_KIND_FIELD_RANGE condition
inline std::string range_entry(const RangeBounds &b)
{
    std::string s(BSG_RANGE_ENTRY_BYTES, '\0');
    const uint64_t lo = b.has_lo ? (uint64_t)b.lo : 0, hi = b.has_hi ? (uint64_t)b.hi : 0;
    for (int i = 0; i < 8; ++i) { s[i] = (char)(lo >> (8 * i)); s[8 + i] = (char)(hi >> (8 * i)); }
    s[16] = (char)b.flags();
    return s;
}

// The tree as the tail of a device row-matcher program (bsg_match_rows_range).  nil condition => TRUE, empty And => TRUE, empty Or =>
// FALSE, unknown node => FALSE, an empty field => FALSE, as RangeRowMatcher::eval.
inline void emit_range_program(const RangeExpression &e, std::vector<uint32_t> &kinds, std::vector<std::string> &fields,
                               std::vector<std::string> &tokens, std::vector<uint32_t> &prog_ops)
{
    switch (e.type) {
    case RegexType::Condition:
        if (!e.has_condition) { prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0)); return; }
        if (e.field.empty()) { prog_ops.push_back(BSG_OP(BSG_OP_FALSE, 0)); return; }
        prog_ops.push_back(BSG_OP(BSG_OP_TERM, (uint32_t)kinds.size()));
        kinds.push_back(BSG_KIND_FIELD_RANGE);
        fields.push_back(e.field);
        tokens.push_back(range_entry(e.bounds));
        return;
    case RegexType::And:
    case RegexType::Or:
        if (e.children.empty()) { prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_TRUE : BSG_OP_FALSE, 0)); return; }
        for (const RangeExpression &c : e.children) emit_range_program(c, kinds, fields, tokens, prog_ops);
        prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_AND : BSG_OP_OR, (uint32_t)e.children.size()));
        return;
    default:
        prog_ops.push_back(BSG_OP(BSG_OP_FALSE, 0));
    }
}

// ---- the exact row test ----
class RangeRowMatcher {
public:
    explicit RangeRowMatcher(const RangeExpression *e)
    {
        if (!e) return;
        root_ = *e; has_root_ = true;
        collect(root_);
    }
    bool match(std::string_view row)
    {
        if (!has_root_) return true;
        sat_.assign(conds_.size(), 0);
        const bool whole = walker_.walk(row, [&](const Emission &em) {
            if (!em.is_leaf || em.type != JType::Number) return true;
            bool parsed = false, ok = false;
            for (size_t i = 0; i < conds_.size(); ++i) {
                if (sat_[i] || conds_[i]->field.empty() || em.path != conds_[i]->field) continue;
                if (!parsed) { ok = parse_decimal_literal(em.text, lit_); parsed = true; }
                if (ok && literal_inside(lit_, conds_[i]->bounds)) sat_[i] = 1;
            }
            return true;
        });
        if (!whole) return false;              // not valid JSON: no row of the store
        size_t next = 0;
        return eval(root_, next);
    }

private:
    RangeExpression root_;
    bool has_root_ = false;
    std::vector<const RangeExpression *> conds_;       // pre-order, matching eval()'s traversal
    std::vector<uint8_t> sat_;
    DecimalLiteral lit_;
    PathWalker walker_;
    void collect(const RangeExpression &e)
    {
        if (e.type == RegexType::Condition) { if (e.has_condition) conds_.push_back(&e); return; }
        for (auto &c : e.children) collect(c);
    }
    // nil condition => true, empty Or => false, empty And => true, unknown node => false (as the regex tree)
    bool eval(const RangeExpression &e, size_t &next) const
    {
        switch (e.type) {
        case RegexType::Condition: return !e.has_condition ? true : (bool)sat_[next++];
        case RegexType::And: { bool r = true; for (auto &c : e.children) r = eval(c, next) && r; return r; }
        case RegexType::Or: { bool r = false; for (auto &c : e.children) r = eval(c, next) || r; return r; }
        default: return false;
        }
    }
};

}  // namespace bsh
