// substring.hpp — substring conditions: "some leaf's text contains the needle".
//   * fold_text: fold(x) = strings.ToLower(x) under a tokenizer with kLower (to_lower per rune, text.hpp), else x.
//   * substring_terms(needle, tok): the tokens every row that contains the needle must hold — what the bloom side prunes with.
//     The folded needle is split at the tokenizer's separators (tested on the folded runes).  A word is WHOLE when the needle has a
//     separator on both of its sides, else PARTIAL (the text may continue it).  Terms:
//         whole    ngram 0: the word              ngram n: grams(word, n)
//         partial  ngram 0: nothing               ngram n: nothing if runes(word) < n, else all its n-rune windows
//     deduplicated, in first-occurrence order.  No false negatives: a whole word of the needle is a whole word of the text; a
//     partial word e with >= n runes lies inside a text word W whose tokens are its windows (which include e's) when W has more
//     than n runes, and else W = e.
//   * SubstringExpression: CONDITION | AND | OR over {"Field": string or absent, "Needle": string}, shaped as RegexExpression.
//   * substring_guard: the tree as a BloomExpression over the terms (And(Token ..) / And(FieldToken ..) per condition; a field
//     condition without terms is Field(field); an any-field condition without terms is the nil condition, which is always true: it is
//     dropped from an And and KEPT in an Or, which it makes true).
//   * SubstringRowMatcher: the exact test per row (the matcher of fallback rows; the device tests compare with it): a condition holds
//     when a leaf (FieldSubstring: a leaf whose path EQUALS the field, FieldToken's rule) has a candidate text T (leafTokenInput: a
//     string's decoded text, a number's raw literal, true / false; never null, never a key) with bytes.Contains(fold(T), fold(needle)).
//     Separators and the n-gram width play no part in the exact test.
// What the device call shares with this file (the needle's limits and folding, the shift-and tables of match.hip.h's SubLane):
// substring_pack.hpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "expression.hpp"
#include "substring_pack.hpp"
#include "text.hpp"
#include "walker.hpp"

namespace bsh {

inline std::vector<std::string> substring_terms(std::string_view needle, const Tokenizer &t)
{
    std::vector<std::string> terms;
    const std::string f = fold_text(needle, t.lower());
    const unsigned char *p = reinterpret_cast<const unsigned char *>(f.data());
    auto add = [&](std::string_view s) {
        for (const std::string &have : terms) if (have == s) return true;
        terms.emplace_back(s);
        return true;
    };
    auto word = [&](size_t a, size_t b, bool whole) {
        const std::string_view w(f.data() + a, b - a);
        if (t.ngram == 0) { if (whole) add(w); return; }
        size_t runes = 0;
        for (size_t i = 0, width; i < w.size(); i += width, ++runes) (void)decode_rune(p + a + i, w.size() - i, width);
        if (!whole && runes < t.ngram) return;
        for_each_gram(w, t.ngram, add);
    };
    size_t start = 0;
    bool in_word = false, seen_sep = false, sep_before = false;   // sep_before: the current word began behind a separator
    for (size_t i = 0; i < f.size();) {
        size_t width;
        const uint32_t r = decode_rune(p + i, f.size() - i, width);
        if (t.is_sep(r)) {
            if (in_word) word(start, i, sep_before);
            in_word = false;
            seen_sep = true;
        } else if (!in_word) {
            in_word = true;
            start = i;
            sep_before = seen_sep;
        }
        i += width;
    }
    if (in_word) word(start, f.size(), false);                    // nothing ends the last word: the text may continue it
    return terms;
}

// ---- the query tree ----
struct SubstringExpression {
    RegexType type = RegexType::Unknown;       // CONDITION | AND | OR, as the regex tree
    bool has_condition = false, has_field = false;
    std::string field, needle;
    std::vector<SubstringExpression> children;
};
inline SubstringExpression Substring(std::string needle)
{
    SubstringExpression e; e.type = RegexType::Condition; e.has_condition = true; e.needle = std::move(needle);
    return e;
}
inline SubstringExpression FieldSubstring(std::string field, std::string needle)
{
    SubstringExpression e = Substring(std::move(needle)); e.has_field = true; e.field = std::move(field);
    return e;
}
inline bool substring_expression_from_json(const JNode &n, SubstringExpression &out)
{
    if (n.type != JType::Object) return false;
    const JNode *t = n.get("ExpressionType");
    const std::string ts = (t && t->type == JType::String) ? t->text : "";
    out.type = ts == "CONDITION" ? RegexType::Condition : ts == "AND" ? RegexType::And : ts == "OR" ? RegexType::Or : RegexType::Unknown;
    const JNode *c = n.get("Condition");
    out.has_condition = c && c->type == JType::Object;
    if (out.has_condition) {
        const JNode *f = c->get("Field"), *nd = c->get("Needle");
        out.has_field = f && f->type == JType::String;
        out.field = out.has_field ? f->text : "";
        out.needle = (nd && nd->type == JType::String) ? nd->text : "";
    }
    const JNode *kids = n.get("Children");
    if (kids && kids->type == JType::Array) {
        out.children.resize(kids->items.size());
        for (size_t i = 0; i < kids->items.size(); ++i)
            if (!substring_expression_from_json(kids->items[i], out.children[i])) return false;
    }
    return true;
}
// every needle of the tree: Ok, or the first status that is not
inline NeedleStatus check_needles(const SubstringExpression &e, const Tokenizer &t)
{
    if (e.type == RegexType::Condition) {
        std::string folded;
        return e.has_condition ? fold_needle(e.needle, t, folded) : NeedleStatus::Ok;
    }
    for (const SubstringExpression &c : e.children) {
        const NeedleStatus s = check_needles(c, t);
        if (s != NeedleStatus::Ok) return s;
    }
    return NeedleStatus::Ok;
}

// The guard of a (sub)tree; false = the nil expression (always true).
inline bool substring_to_bloom_expression(const SubstringExpression &e, const Tokenizer &t, BloomExpression &out)
{
    switch (e.type) {
    case RegexType::Condition: {
        if (!e.has_condition) return false;
        const std::vector<std::string> terms = substring_terms(e.needle, t);
        if (terms.empty()) {
            if (!e.has_field) return false;
            out = Field(e.field);
            return true;
        }
        std::vector<BloomExpression> kids;
        for (const std::string &s : terms) kids.push_back(e.has_field ? FieldToken(e.field, s) : Token(s));
        out = And(std::move(kids));
        return true;
    }
    case RegexType::And:
    case RegexType::Or: {
        const bool is_and = e.type == RegexType::And;
        out = BloomExpression{};
        out.type = is_and ? ExprType::And : ExprType::Or;
        for (const SubstringExpression &c : e.children) {
            BloomExpression child;
            if (substring_to_bloom_expression(c, t, child)) out.children.push_back(std::move(child));
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
inline bool substring_guard(const SubstringExpression *sub, const Tokenizer &t, BloomExpression &out)
{
    return sub && substring_to_bloom_expression(*sub, t, out);
}

// The tree as the tail of a device row-matcher program (bsg_match_rows_substr): conditions appended to kinds / fields / tokens (a
// Substring condition keeps an empty field, both keep the RAW needle as the token string), ops to prog_ops.  nil condition => TRUE,
// empty And => TRUE, empty Or => FALSE, unknown node => FALSE, as SubstringRowMatcher::eval.
inline void emit_substring_program(const SubstringExpression &e, std::vector<uint32_t> &kinds, std::vector<std::string> &fields,
                                   std::vector<std::string> &tokens, std::vector<uint32_t> &prog_ops)
{
    switch (e.type) {
    case RegexType::Condition:
        if (!e.has_condition) { prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0)); return; }
        prog_ops.push_back(BSG_OP(BSG_OP_TERM, (uint32_t)kinds.size()));
        kinds.push_back(e.has_field ? BSG_KIND_FIELD_SUBSTRING : BSG_KIND_SUBSTRING);
        fields.push_back(e.has_field ? e.field : std::string());
        tokens.push_back(e.needle);
        return;
    case RegexType::And:
    case RegexType::Or:
        if (e.children.empty()) { prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_TRUE : BSG_OP_FALSE, 0)); return; }
        for (const SubstringExpression &c : e.children) emit_substring_program(c, kinds, fields, tokens, prog_ops);
        prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_AND : BSG_OP_OR, (uint32_t)e.children.size()));
        return;
    default:
        prog_ops.push_back(BSG_OP(BSG_OP_FALSE, 0));
    }
}

// ---- the exact row test ----
class SubstringRowMatcher {
public:
    explicit SubstringRowMatcher(const SubstringExpression *e, const Tokenizer &tok = Tokenizer()) : lower_(tok.lower())
    {
        if (!e) return;
        root_ = *e; has_root_ = true;
        collect(root_, tok);
    }
    bool valid() const { return status_ == NeedleStatus::Ok; }
    NeedleStatus status() const { return status_; }
    bool match(std::string_view row)
    {
        if (!has_root_) return true;
        sat_.assign(conds_.size(), 0);
        walker_.walk(row, [&](const Emission &em) {
            if (!em.is_leaf || !em.has_text) return true;
            bool folded = false;
            for (size_t i = 0; i < conds_.size(); ++i) {
                if (sat_[i] || (conds_[i]->has_field && em.path != conds_[i]->field)) continue;
                if (!folded) { fold_ = fold_text(em.text, lower_); folded = true; }
                if (fold_.find(needles_[i]) != std::string::npos) sat_[i] = 1;
            }
            return true;
        });
        size_t next = 0;
        return eval(root_, next);
    }

private:
    SubstringExpression root_;
    bool has_root_ = false, lower_ = true;
    NeedleStatus status_ = NeedleStatus::Ok;
    std::vector<const SubstringExpression *> conds_;   // pre-order, matching eval()'s traversal
    std::vector<std::string> needles_;                 // folded
    std::vector<uint8_t> sat_;
    std::string fold_;
    PathWalker walker_;
    void collect(const SubstringExpression &e, const Tokenizer &tok)
    {
        if (e.type == RegexType::Condition) {
            if (!e.has_condition) return;
            conds_.push_back(&e);
            needles_.emplace_back();
            const NeedleStatus s = fold_needle(e.needle, tok, needles_.back());
            if (s != NeedleStatus::Ok && status_ == NeedleStatus::Ok) status_ = s;
            return;
        }
        for (auto &c : e.children) collect(c, tok);
    }
    // nil condition => true, empty Or => false, empty And => true, unknown node => false (as the regex tree)
    bool eval(const SubstringExpression &e, size_t &next) const
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
