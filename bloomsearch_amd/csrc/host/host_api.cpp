// host_api.cpp — C-ABI shims of include/bloomsearch_host.h over the header-only host mirror.
#include "bloomsearch_host.h"

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>

#include "engine.hpp"
#include "regex_dfa.hpp"
#include "minmax.hpp"
#include "partition.hpp"
#include "range.hpp"
#include "substring.hpp"

using namespace bsh;

struct bsh_entry_sets { BloomEntrySets sets; };
struct bsh_batch { QueryBatch batch; };
struct bse_engine {
    std::unique_ptr<BloomSearchEngine> eng;
    std::string err;
};

namespace {

int32_t give(const std::string &s, char **out, uint64_t *out_len)
{
    char *p = static_cast<char *>(malloc(s.size() + 1));
    if (!p) return BSH_E_INVALID;
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    *out = p;
    if (out_len) *out_len = s.size();
    return 0;
}

void json_escape(std::string &out, std::string_view s)
{
    static const char *hex = "0123456789abcdef";
    out.push_back('"');
    for (unsigned char c : s) {
        switch (c) {
        case '"': out += "\\\""; break;
        case '\\': out += "\\\\"; break;
        case '\n': out += "\\n"; break;
        case '\r': out += "\\r"; break;
        case '\t': out += "\\t"; break;
        default:
            if (c < 0x20) { out += "\\u00"; out.push_back(hex[c >> 4]); out.push_back(hex[c & 15]); }
            else out.push_back((char)c);
        }
    }
    out.push_back('"');
}

bool parse_expression_json(const char *json, uint64_t len, BloomExpression &expr, bool &is_nil)
{
    is_nil = true;
    std::string_view sv(json ? json : "", json ? len : 0);
    size_t a = 0;
    while (a < sv.size() && (sv[a] == ' ' || sv[a] == '\n' || sv[a] == '\t' || sv[a] == '\r')) ++a;
    if (a == sv.size()) return true;
    JNode dom;
    if (!parse_dom(sv, dom)) return false;
    if (dom.type == JType::Null) return true;
    is_nil = false;
    return expression_from_json(dom, expr);
}

// a C spec -> the host mirror's Tokenizer (NULL = the default); false for an invalid spec (bloomgpu.h bsg_tokenizer)
bool tokenizer_from(const bsg_tokenizer *in, Tokenizer &out)
{
    out = Tokenizer();
    if (!in) return true;
    if ((in->sep_ascii[0] & 1u) || in->reserved || (in->flags & ~(BSG_TOK_UNICODE_SPACE | BSG_TOK_LOWER | BSG_TOK_NGRAM_MASK))) return false;
    const uint32_t ngram = (in->flags & BSG_TOK_NGRAM_MASK) >> BSG_TOK_NGRAM_SHIFT;
    if (!Tokenizer::valid_ngram(ngram)) return false;
    out.sep[0] = in->sep_ascii[0];
    out.sep[1] = in->sep_ascii[1];
    out.flags = in->flags & (BSG_TOK_UNICODE_SPACE | BSG_TOK_LOWER);
    out.ngram = ngram;
    return true;
}

// "Tokenizer": {"Separators": "...", "UnicodeSpace": bool, "Lower": bool, "Ngram": int}; a missing key is Go's zero value ("", false, 0).
// false: not an object, a separator that is NUL or not ASCII, an "Ngram" that is not the integer 0, 2, 3 or 4.
bool tokenizer_from_json(const JNode &n, Tokenizer &out)
{
    if (n.type != JType::Object) return false;
    out.sep[0] = out.sep[1] = 0;
    out.flags = 0;
    out.ngram = 0;
    if (const JNode *g = n.get("Ngram")) {
        if (g->type != JType::Number || g->text.size() != 1 || g->text[0] < '0' || g->text[0] > '9' || !Tokenizer::valid_ngram(g->text[0] - '0')) return false;
        out.ngram = g->text[0] - '0';
    }
    if (const JNode *s = n.get("Separators")) {
        if (s->type != JType::String) return false;
        for (unsigned char c : s->text) {
            if (c == 0 || c >= 0x80) return false;
            out.sep[c >> 6] |= 1ull << (c & 63);
        }
    }
    if (const JNode *u = n.get("UnicodeSpace")) { if (u->type == JType::True) out.flags |= Tokenizer::kUnicodeSpace; }
    if (const JNode *l = n.get("Lower")) { if (l->type == JType::True) out.flags |= Tokenizer::kLower; }
    return true;
}

uint64_t num_or(const JNode &cfg, const char *key, uint64_t dflt)
{
    const JNode *n = cfg.get(key);
    if (!n || n->type != JType::Number) return dflt;
    return strtoull(n->text.c_str(), nullptr, 10);
}

}  // namespace

extern "C" {

void bsh_free(void *p) { free(p); }

int32_t bsh_tokenize(const uint8_t *text, uint64_t len, char **out, uint64_t *out_len)
{
    std::string joined, tok;
    for_each_word(std::string_view(reinterpret_cast<const char *>(text), len), [&](std::string_view w) {
        tok.clear();
        append_folded_word(tok, w);
        if (!joined.empty()) joined.push_back('\n');
        joined += tok;
        return true;
    });
    return give(joined, out, out_len);
}

int32_t bsh_tokenize_with(const uint8_t *text, uint64_t len, const bsg_tokenizer *tok, uint8_t **out, uint64_t *out_len)
{
    Tokenizer t;
    if (!out || !tokenizer_from(tok, t)) return BSH_E_INVALID;
    std::string packed, buf;
    for_each_token(std::string_view(reinterpret_cast<const char *>(text), len), t, buf, [&](std::string_view w) {
        const uint32_t n = (uint32_t)w.size();
        for (int i = 0; i < 4; ++i) packed.push_back((char)(n >> (8 * i)));
        packed.append(w);
        return true;
    });
    return give(packed, reinterpret_cast<char **>(out), out_len);
}

bsh_entry_sets *bsh_entry_sets_new(void) { return new bsh_entry_sets(); }
void bsh_entry_sets_free(bsh_entry_sets *s) { delete s; }

int32_t bsh_entry_sets_index_row(bsh_entry_sets *s, const uint8_t *row, uint64_t len)
{
    if (!s) return BSH_E_INVALID;
    return s->sets.index_row(std::string_view(reinterpret_cast<const char *>(row), len)) ? 0 : BSH_E_INVALID;
}

int32_t bsh_entry_sets_index_row_with(bsh_entry_sets *s, const uint8_t *row, uint64_t len, const bsg_tokenizer *tok)
{
    Tokenizer t;
    if (!s || !tokenizer_from(tok, t)) return BSH_E_INVALID;
    s->sets.tok = t;
    const bool ok = s->sets.index_row(std::string_view(reinterpret_cast<const char *>(row), len));
    s->sets.tok = Tokenizer();
    return ok ? 0 : BSH_E_INVALID;
}

int32_t bsh_entry_sets_union_into(const bsh_entry_sets *src, bsh_entry_sets *dst)
{
    if (!src || !dst) return BSH_E_INVALID;
    src->sets.union_into(dst->sets);
    return 0;
}

void bsh_entry_sets_counts(const bsh_entry_sets *s, uint64_t counts[3])
{
    const BloomEntryCounts c = s->sets.counts();
    counts[0] = c.fields; counts[1] = c.tokens; counts[2] = c.field_tokens;
}

int32_t bsh_entry_sets_export_sizes(const bsh_entry_sets *s, uint32_t kind, uint64_t *n_entries, uint64_t *n_bytes)
{
    if (!s || kind > 2) return BSH_E_INVALID;
    const auto &set = s->sets.set_of(kind);
    uint64_t b = 0;
    for (auto &e : set) b += e.size();
    *n_entries = set.size();
    *n_bytes = b;
    return 0;
}

int32_t bsh_entry_sets_export(const bsh_entry_sets *s, uint32_t kind, uint8_t *bytes, uint32_t *offsets)
{
    if (!s || kind > 2) return BSH_E_INVALID;
    uint32_t pos = 0, i = 0;
    offsets[0] = 0;
    for (auto &e : s->sets.set_of(kind)) {
        memcpy(bytes + pos, e.data(), e.size());
        pos += (uint32_t)e.size();
        offsets[++i] = pos;
    }
    return 0;
}

bsh_batch *bsh_batch_new(void) { return new bsh_batch(); }
void bsh_batch_free(bsh_batch *b) { delete b; }

int32_t bsh_batch_add_query(bsh_batch *b, const char *expr_json, uint64_t len)
{
    if (!b) return BSH_E_INVALID;
    BloomExpression e;
    bool nil = true;
    if (!parse_expression_json(expr_json, len, e, nil)) return BSH_E_INVALID;
    b->batch.add_query(nil ? nullptr : &e);
    return 0;
}

void bsh_batch_sizes(const bsh_batch *b, uint32_t *n_queries, uint32_t *n_terms, uint32_t *n_ops, uint64_t *term_bytes)
{
    uint64_t tb = 0;
    for (auto &s : b->batch.term_strings) tb += s.size();
    *n_queries = b->batch.n_queries();
    *n_terms = (uint32_t)b->batch.term_strings.size();
    *n_ops = (uint32_t)b->batch.prog_ops.size();
    *term_bytes = tb;
}

int32_t bsh_batch_export(const bsh_batch *b, uint8_t *term_bytes, uint32_t *term_offsets, uint32_t *term_kinds,
                         uint32_t *prog_ops, uint32_t *prog_off)
{
    if (!b) return BSH_E_INVALID;
    uint32_t pos = 0;
    term_offsets[0] = 0;
    for (size_t i = 0; i < b->batch.term_strings.size(); ++i) {
        const std::string &s = b->batch.term_strings[i];
        memcpy(term_bytes + pos, s.data(), s.size());
        pos += (uint32_t)s.size();
        term_offsets[i + 1] = pos;
        term_kinds[i] = b->batch.term_kinds[i];
    }
    if (!b->batch.prog_ops.empty()) memcpy(prog_ops, b->batch.prog_ops.data(), b->batch.prog_ops.size() * 4);
    memcpy(prog_off, b->batch.prog_off.data(), b->batch.prog_off.size() * 4);
    return 0;
}

int32_t bsh_match_row(const char *expr_json, uint64_t expr_len, const uint8_t *row, uint64_t row_len)
{
    BloomExpression e;
    bool nil = true;
    if (!parse_expression_json(expr_json, expr_len, e, nil)) return BSH_E_INVALID;
    RowMatcher m(nil ? nullptr : &e);
    return m.match(std::string_view(reinterpret_cast<const char *>(row), row_len)) ? 1 : 0;
}

int32_t bsh_match_row_with(const char *expr_json, uint64_t expr_len, const uint8_t *row, uint64_t row_len, const bsg_tokenizer *tok)
{
    BloomExpression e;
    bool nil = true;
    Tokenizer t;
    if (!tokenizer_from(tok, t) || !parse_expression_json(expr_json, expr_len, e, nil)) return BSH_E_INVALID;
    RowMatcher m(nil ? nullptr : &e, t);
    return m.match(std::string_view(reinterpret_cast<const char *>(row), row_len)) ? 1 : 0;
}

namespace {
void expression_to_json(const BloomExpression &e, std::string &out)
{
    out += "{\"ExpressionType\":";
    out += e.type == ExprType::Condition ? "\"CONDITION\"" : e.type == ExprType::And ? "\"AND\"" : e.type == ExprType::Or ? "\"OR\"" : "\"?\"";
    if (e.type == ExprType::Condition) {
        out += ",\"Condition\":";
        if (!e.has_condition) out += "null";
        else {
            const char *t = e.condition.type == CondType::Field ? "FIELD" : e.condition.type == CondType::Token ? "TOKEN"
                          : e.condition.type == CondType::FieldToken ? "FIELD_TOKEN" : "?";
            out += std::string("{\"Type\":\"") + t + "\",\"Field\":";
            json_escape(out, e.condition.field);
            out += ",\"Token\":";
            json_escape(out, e.condition.token);
            out += "}";
        }
    } else {
        out += ",\"Children\":[";
        for (size_t i = 0; i < e.children.size(); ++i) { if (i) out.push_back(','); expression_to_json(e.children[i], out); }
        out += "]";
    }
    out += "}";
}
bool parse_regex_json(const char *json, uint64_t len, RegexExpression &e, bool &nil)
{
    nil = true;
    std::string_view sv(json ? json : "", json ? len : 0);
    if (sv.empty()) return true;
    JNode dom;
    if (!parse_dom(sv, dom)) return false;
    if (dom.type == JType::Null) return true;
    if (!regex_expression_from_json(dom, e)) return false;
    nil = false;
    return true;
}
}  // namespace

// pruneBloomQuery (query_exec.go:220): AndBloomQueries(bloom, RegexFieldGuardBloomQuery(regex)) as JSON ("null" = nil query)
int32_t bsh_prune_query(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len, char **out, uint64_t *out_len)
{
    BloomExpression b, guard, pruned;
    RegexExpression r;
    bool bnil = true, rnil = true;
    if (!parse_expression_json(bloom_json, bloom_len, b, bnil) || !parse_regex_json(regex_json, regex_len, r, rnil)) return BSH_E_INVALID;
    const bool has_guard = regex_field_guard(rnil ? nullptr : &r, guard);
    std::string s = "null";
    if (and_bloom_queries(bnil ? nullptr : &b, has_guard ? &guard : nullptr, pruned)) { s.clear(); expression_to_json(pruned, s); }
    return give(s, out, out_len);
}

namespace {
bool parse_substring_json(const char *json, uint64_t len, SubstringExpression &e, bool &nil)
{
    nil = true;
    std::string_view sv(json ? json : "", json ? len : 0);
    if (sv.empty()) return true;
    JNode dom;
    if (!parse_dom(sv, dom)) return false;
    if (dom.type == JType::Null) return true;
    if (!substring_expression_from_json(dom, e)) return false;
    nil = false;
    return true;
}
int32_t needle_status(NeedleStatus s) { return s == NeedleStatus::Ok ? 0 : s == NeedleStatus::TooLong ? BSG_E_UNSUPPORTED : BSH_E_INVALID; }
}  // namespace

// substring_terms (substring.hpp): the tokens a row that contains the needle must hold, packed as bsh_tokenize_with packs tokens
int32_t bsh_substring_terms(const uint8_t *needle, uint64_t len, const bsg_tokenizer *tok, uint8_t **out, uint64_t *out_len)
{
    Tokenizer t;
    if (!out || (len && !needle) || !tokenizer_from(tok, t)) return BSH_E_INVALID;
    const std::string_view nd(reinterpret_cast<const char *>(needle), len);
    std::string folded, packed;
    if (int32_t rc = needle_status(fold_needle(nd, t, folded))) return rc;
    for (const std::string &w : substring_terms(nd, t)) {
        const uint32_t n = (uint32_t)w.size();
        for (int i = 0; i < 4; ++i) packed.push_back((char)(n >> (8 * i)));
        packed.append(w);
    }
    return give(packed, reinterpret_cast<char **>(out), out_len);
}

// bsh_prune_query with the substring tree's guard as a third side: And(bloom, regex field guard, substring guard)
int32_t bsh_prune_query_sub(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len, const char *substring_json,
                            uint64_t substring_len, const bsg_tokenizer *tok, char **out, uint64_t *out_len)
{
    BloomExpression b, guard, sguard, two, pruned;
    RegexExpression r;
    SubstringExpression sx;
    Tokenizer t;
    bool bnil = true, rnil = true, snil = true;
    if (!tokenizer_from(tok, t) || !parse_expression_json(bloom_json, bloom_len, b, bnil) || !parse_regex_json(regex_json, regex_len, r, rnil) ||
        !parse_substring_json(substring_json, substring_len, sx, snil))
        return BSH_E_INVALID;
    if (!snil) if (int32_t rc = needle_status(check_needles(sx, t))) return rc;
    const bool has_guard = regex_field_guard(rnil ? nullptr : &r, guard);
    const bool has_two = and_bloom_queries(bnil ? nullptr : &b, has_guard ? &guard : nullptr, two);
    const bool has_sub = substring_guard(snil ? nullptr : &sx, t, sguard);
    std::string s = "null";
    if (and_bloom_queries(has_two ? &two : nullptr, has_sub ? &sguard : nullptr, pruned)) { s.clear(); expression_to_json(pruned, s); }
    return give(s, out, out_len);
}

// the substring half of the final row test (substring.hpp SubstringRowMatcher): 1 match, 0 no match, < 0 invalid arguments / needle
int32_t bsh_match_row_substring(const char *substring_json, uint64_t substring_len, const uint8_t *row, uint64_t row_len, const bsg_tokenizer *tok)
{
    SubstringExpression sx;
    Tokenizer t;
    bool nil = true;
    if (!tokenizer_from(tok, t) || !parse_substring_json(substring_json, substring_len, sx, nil)) return BSH_E_INVALID;
    SubstringRowMatcher m(nil ? nullptr : &sx, t);
    if (int32_t rc = needle_status(m.status())) return rc;
    return m.match(std::string_view(reinterpret_cast<const char *>(row), row_len)) ? 1 : 0;
}

namespace {
bool parse_range_json(const char *json, uint64_t len, RangeExpression &e, bool &nil)
{
    nil = true;
    std::string_view sv(json ? json : "", json ? len : 0);
    if (sv.empty()) return true;
    JNode dom;
    if (!parse_dom(sv, dom)) return false;
    if (dom.type == JType::Null) return true;
    if (!range_expression_from_json(dom, e)) return false;
    nil = false;
    return true;
}
}  // namespace

// bsh_prune_query_sub with the range tree's guard as a fourth side
int32_t bsh_prune_query_range(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len, const char *substring_json,
                              uint64_t substring_len, const char *range_json, uint64_t range_len, const bsg_tokenizer *tok, char **out, uint64_t *out_len)
{
    BloomExpression b, guard, sguard, rguard, two, three, pruned;
    RegexExpression r;
    SubstringExpression sx;
    RangeExpression rg;
    Tokenizer t;
    bool bnil = true, rnil = true, snil = true, gnil = true;
    if (!tokenizer_from(tok, t) || !parse_expression_json(bloom_json, bloom_len, b, bnil) || !parse_regex_json(regex_json, regex_len, r, rnil) ||
        !parse_substring_json(substring_json, substring_len, sx, snil) || !parse_range_json(range_json, range_len, rg, gnil))
        return BSH_E_INVALID;
    if (!snil) if (int32_t rc = needle_status(check_needles(sx, t))) return rc;
    const bool has_guard = regex_field_guard(rnil ? nullptr : &r, guard);
    const bool has_two = and_bloom_queries(bnil ? nullptr : &b, has_guard ? &guard : nullptr, two);
    const bool has_sub = substring_guard(snil ? nullptr : &sx, t, sguard);
    const bool has_three = and_bloom_queries(has_two ? &two : nullptr, has_sub ? &sguard : nullptr, three);
    const bool has_range = range_guard(gnil ? nullptr : &rg, rguard);
    std::string s = "null";
    if (and_bloom_queries(has_three ? &three : nullptr, has_range ? &rguard : nullptr, pruned)) { s.clear(); expression_to_json(pruned, s); }
    return give(s, out, out_len);
}

// the range half of the final row test (range.hpp RangeRowMatcher): 1 match, 0 no match, < 0 invalid arguments
int32_t bsh_match_row_range(const char *range_json, uint64_t range_len, const uint8_t *row, uint64_t row_len)
{
    RangeExpression rg;
    bool nil = true;
    if ((row_len && !row) || !parse_range_json(range_json, range_len, rg, nil)) return BSH_E_INVALID;
    RangeRowMatcher m(nil ? nullptr : &rg);
    return m.match(std::string_view(reinterpret_cast<const char *>(row), row_len)) ? 1 : 0;
}

// one row's MinMax contributions folded into inout[n_fields] (minmax.hpp minmax_row): 0, or < 0 for invalid fields / a row that is no JSON object
int32_t bsh_minmax_row(const uint8_t *row, uint64_t len, const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields, bsg_minmax *inout)
{
    MinMaxFieldNames f;
    std::string why;
    if ((len && !row) || !inout || !f.unpack(field_bytes, field_off, n_fields, why)) return BSH_E_INVALID;
    return minmax_row(std::string_view(reinterpret_cast<const char *>(row), len), f.names, inout) ? 0 : BSH_E_INVALID;
}

// one row's slot of a bucketed hit count (minmax.hpp hist_row_slot): 0, or < 0 for invalid arguments / a row that is no JSON object
int32_t bsh_hist_row(const uint8_t *row, uint64_t len, const uint8_t *field, uint32_t field_len, int64_t origin, uint64_t width, uint32_t n_buckets,
                     uint32_t *out_slot)
{
    if ((len && !row) || !field || field_len == 0 || field_len > BSG_MINMAX_MAX_NAME || width == 0 || n_buckets == 0 || n_buckets > BSG_HIST_MAX_BUCKETS ||
        !out_slot)
        return BSH_E_INVALID;
    uint32_t slot = 0;
    if (!hist_row_slot(std::string_view(reinterpret_cast<const char *>(row), len), std::string(reinterpret_cast<const char *>(field), field_len), origin, width,
                       n_buckets, slot))
        return BSH_E_INVALID;
    *out_slot = slot;
    return 0;
}

// one row's partition text (partition.hpp partition_key: the first top-level member with the key; escapes decoded): 0, *out_len = its
// length, the first min(cap, length) bytes in out; < 0 for an empty or over-long name or a row that is not one valid JSON object
int32_t bsh_partition_key(const uint8_t *row, uint64_t len, const uint8_t *name, uint32_t name_len, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
    if ((len && !row) || !name || name_len == 0 || name_len > BSG_PARTITION_MAX_NAME || !out_len || (cap && !out)) return BSH_E_INVALID;
    std::string text;
    if (!partition_key(std::string_view(reinterpret_cast<const char *>(row), len), std::string_view(reinterpret_cast<const char *>(name), name_len), text))
        return BSH_E_INVALID;
    *out_len = text.size();
    if (!text.empty() && cap) memcpy(out, text.data(), std::min<uint64_t>(cap, text.size()));
    return 0;
}

// EvaluateMinMaxCondition: 1 the block may hold a matching value, 0 it cannot, < 0 invalid arguments (an absent index included)
int32_t bsh_minmax_eval(const bsg_minmax *index, uint32_t op, int64_t value, const int64_t *values, uint32_t n_values, int64_t min, int64_t max)
{
    if (!index || !index->present || op >= MM_OP_COUNT || (n_values && !values)) return BSH_E_INVALID;
    return minmax_eval(index->min, index->max, op, value, values, n_values, min, max) ? 1 : 0;
}

// evaluatePrefilterExpression on one block: its partition id and the indexes it carries, named by the packed fields
int32_t bsh_prefilter_eval(const char *prefilter_json, uint64_t len, const uint8_t *partition_id, uint64_t partition_len, const uint8_t *field_bytes,
                           const uint32_t *field_off, uint32_t n_fields, const bsg_minmax *indexes)
{
    if ((len && !prefilter_json) || (partition_len && !partition_id) || (n_fields && (!field_bytes || !field_off || !indexes))) return BSH_E_INVALID;
    const std::string_view text(prefilter_json ? prefilter_json : "", len);
    std::map<std::string, bsg_minmax> have;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (field_off[f + 1] < field_off[f]) return BSH_E_INVALID;
        if (indexes[f].present) have[std::string((const char *)field_bytes + field_off[f], field_off[f + 1] - field_off[f])] = indexes[f];
    }
    if (text.empty() || text == "null") return 1;                  // a nil expression: every block passes
    JNode n;
    PrefilterExpression e;
    if (!parse_dom(text, n)) return BSH_E_INVALID;
    if (n.type == JType::Null) return 1;
    if (!prefilter_from_json(n, e)) return BSH_E_INVALID;
    const PrefilterBlock b{std::string_view((const char *)partition_id, partition_len), &have};
    return prefilter_eval(e, b) ? 1 : 0;
}

// the regex half of matchRowBytes (row_matcher.go:548-573): 1 match, 0 no match, < 0 invalid arguments / pattern
int32_t bsh_match_row_regex(const char *regex_json, uint64_t regex_len, const uint8_t *row, uint64_t row_len)
{
    RegexExpression r;
    bool nil = true;
    if (!parse_regex_json(regex_json, regex_len, r, nil)) return BSH_E_INVALID;
    RegexRowMatcher m(nil ? nullptr : &r);
    if (!m.valid()) return BSH_E_INVALID;
    return m.match(std::string_view(reinterpret_cast<const char *>(row), row_len)) ? 1 : 0;
}

// MatchString of one pattern of the device regex subset (regex_dfa.hpp) on one text: 1 / 0 / BSG_E_UNSUPPORTED
int32_t bsh_regex_match(const char *pattern, uint64_t plen, const uint8_t *text, uint64_t tlen)
{
    if ((plen && !pattern) || (tlen && !text)) return BSH_E_INVALID;
    bsh_rx::Dfa d;
    std::string err;
    if (!bsh_rx::compile(std::string_view(pattern ? pattern : "", plen), d, err)) return BSG_E_UNSUPPORTED;
    return bsh_rx::run(d, text, tlen) ? 1 : 0;
}

int32_t bsh_section_encode(const uint64_t *const words[3], const uint64_t m[3], const uint64_t k[3], uint8_t **out, uint64_t *out_len)
{
    FilterView fv[3];
    for (int c = 0; c < 3; ++c) fv[c] = FilterView{words[c], m[c], k[c]};
    const std::vector<uint8_t> sec = encode_filter_section(fv);
    uint8_t *p = static_cast<uint8_t *>(malloc(sec.size()));
    if (!p) return BSH_E_INVALID;
    memcpy(p, sec.data(), sec.size());
    *out = p;
    *out_len = sec.size();
    return 0;
}

int32_t bsh_section_parse(const uint8_t *section, uint64_t len, uint64_t m[3], uint64_t k[3], uint64_t *words[3])
{
    ParsedFilter pf[3];
    const int32_t rc = parse_filter_section(section, len, pf);
    if (rc) return rc;
    for (int c = 0; c < 3; ++c) {
        m[c] = pf[c].present ? pf[c].m : 0;
        k[c] = pf[c].present ? pf[c].k : 0;
        words[c] = nullptr;
        if (pf[c].present) {
            words[c] = static_cast<uint64_t *>(malloc(std::max<size_t>(pf[c].words.size(), 1) * 8));
            memcpy(words[c], pf[c].words.data(), pf[c].words.size() * 8);
        }
    }
    return 0;
}

uint32_t bsh_crc32c(const uint8_t *data, uint64_t len) { return crc32c(data, len); }

// ---- engine ----
int32_t bse_open(const char *config_json, uint64_t len, bsg_ctx *ctx, bse_engine **out)
{
    if (!out) return BSH_E_INVALID;
    *out = nullptr;
    EngineConfig cfg;
    std::string_view sv(config_json ? config_json : "", config_json ? len : 0);
    if (!sv.empty()) {
        JNode dom;
        if (!parse_dom(sv, dom) || dom.type != JType::Object) return BSE_E_INVALID_CONFIG;
        cfg.max_row_group_rows = num_or(dom, "MaxRowGroupRows", cfg.max_row_group_rows);
        cfg.max_row_group_bytes = num_or(dom, "MaxRowGroupBytes", cfg.max_row_group_bytes);
        cfg.max_buffered_rows = num_or(dom, "MaxBufferedRows", cfg.max_buffered_rows);
        cfg.max_buffered_bytes = num_or(dom, "MaxBufferedBytes", cfg.max_buffered_bytes);
        if (const JNode *n = dom.get("BloomFalsePositiveRate")) { if (n->type == JType::Number) cfg.bloom_false_positive_rate = strtod(n->text.c_str(), nullptr); }
        if (const JNode *n = dom.get("PartitionField")) { if (n->type == JType::String) cfg.partition_field = n->text; }
        if (const JNode *n = dom.get("DeviceIngest")) cfg.device_ingest = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceIngestStream")) cfg.device_ingest_stream = n->type == JType::True;
        if (const JNode *n = dom.get("TrustedRows")) cfg.trusted_rows = n->type == JType::True;
        if (const JNode *n = dom.get("DevicePartition")) cfg.device_partition = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatch")) cfg.device_match = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceRegex")) cfg.device_regex = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchRangeText")) cfg.device_match_range_text = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchRangeTextWide")) cfg.device_match_range_text_wide = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchWide")) cfg.device_match_wide = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchWideRows")) cfg.device_match_wide_rows = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchLookup")) cfg.device_match_lookup = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchLookupRows")) cfg.device_match_lookup_rows = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchLookupRegex")) cfg.device_match_lookup_regex = n->type == JType::True;
        if (const JNode *n = dom.get("DeviceMatchHistogram")) cfg.device_match_histogram = n->type == JType::True;
        if (const JNode *n = dom.get("MinMaxIndexes")) {       // ["timestamp", ...]; null or [] = none
            if (n->type != JType::Null && n->type != JType::Array) return BSE_E_INVALID_CONFIG;
            for (const JNode &f : n->items) {
                if (f.type != JType::String) return BSE_E_INVALID_CONFIG;
                cfg.minmax_indexes.push_back(f.text);
            }
        }
        if (const JNode *n = dom.get("Tokenizer")) {
            if (n->type != JType::Null && !tokenizer_from_json(*n, cfg.tokenizer)) return BSE_E_INVALID_CONFIG;
        }
    }
    std::string err;
    if (int32_t rc = BloomSearchEngine::validate(cfg, err)) return rc;
    if (!ctx) return BSH_E_INVALID;     // (after the config: a config is checked without a device)
    auto *e = new bse_engine();
    e->eng = std::make_unique<BloomSearchEngine>(cfg, ctx);
    *out = e;
    return 0;
}

void bse_close(bse_engine *e) { delete e; }
const char *bse_last_error(bse_engine *e) { return e ? e->eng->last_error().c_str() : ""; }
int32_t bse_stop(bse_engine *e) { if (!e) return BSH_E_INVALID; e->eng->stop(); return 0; }

int32_t bse_ingest_rows(bse_engine *e, const uint8_t *ndjson, uint64_t len)
{
    if (!e) return BSH_E_INVALID;
    std::vector<std::string_view> rows;
    std::string_view all(reinterpret_cast<const char *>(ndjson), len);
    size_t pos = 0;
    while (pos < all.size()) {
        size_t nl = all.find('\n', pos);
        if (nl == std::string_view::npos) nl = all.size();
        if (nl > pos) rows.push_back(all.substr(pos, nl - pos));
        pos = nl + 1;
    }
    return e->eng->ingest_rows(rows);
}

int32_t bse_flush(bse_engine *e) { return e ? e->eng->flush() : BSH_E_INVALID; }
int32_t bse_merge(bse_engine *e) { return e ? e->eng->merge() : BSH_E_INVALID; }

namespace {

// one element of bse_query / bse_query_many: {"Bloom":{"Expression":..}|null,"Regex":{"Expression":..}|null} or null
struct ParsedQuery {
    BloomExpression expr;
    RegexExpression regex;
    SubstringExpression sub;
    RangeExpression range;
    PrefilterExpression prefilter;
    bool nil = true, has_regex = false, has_sub = false, has_range = false, has_prefilter = false;
    // "Histogram": {"Field", "Origin", "Width", "Buckets"}: the result holds bucketed hit counts instead of rows
    bool has_hist = false;
    HistSpec hist;
};

// a JSON number that is a plain integer literal within [lo, hi] (no fraction, no exponent)
bool integer_member(const JNode *n, bool is_signed, int64_t &sv, uint64_t &uv)
{
    if (!n || n->type != JType::Number || n->text.empty() || n->text.find_first_of(".eE") != std::string::npos) return false;
    errno = 0;
    char *end = nullptr;
    if (is_signed) sv = strtoll(n->text.c_str(), &end, 10);
    else { if (n->text[0] == '-') return false; uv = strtoull(n->text.c_str(), &end, 10); }
    return errno == 0 && end && *end == 0;
}

int32_t query_from_dom(const JNode &dom, ParsedQuery &q)
{
    if (dom.type == JType::Object) {
        const JNode *bloom = dom.get("Bloom");
        if (bloom && bloom->type == JType::Object) {
            const JNode *ex = bloom->get("Expression");
            if (ex && ex->type == JType::Object) {
                if (!expression_from_json(*ex, q.expr)) return BSE_E_INVALID_QUERY;
                q.nil = false;
            }
        }
        const JNode *rx = dom.get("Regex");
        if (rx && rx->type == JType::Object) {
            const JNode *ex = rx->get("Expression");
            if (ex && ex->type == JType::Object) {
                if (!regex_expression_from_json(*ex, q.regex)) return BSE_E_INVALID_QUERY;
                q.has_regex = true;
            }
        }
        // "Substring": the tree itself, or {"Expression": tree} as the two other members are wrapped
        const JNode *sx = dom.get("Substring");
        if (sx && sx->type == JType::Object) {
            const JNode *ex = sx->get("Expression");
            if (!substring_expression_from_json(ex && ex->type == JType::Object ? *ex : *sx, q.sub)) return BSE_E_INVALID_QUERY;
            q.has_sub = true;
        }
        // "Range": the same two forms
        const JNode *rg = dom.get("Range");
        if (rg && rg->type == JType::Object) {
            const JNode *ex = rg->get("Expression");
            if (!range_expression_from_json(ex && ex->type == JType::Object ? *ex : *rg, q.range)) return BSE_E_INVALID_QUERY;
            q.has_range = true;
        }
        // "Histogram": the bucket spec of bsg_match_rows_wide_hist, with its limits
        const JNode *hg = dom.get("Histogram");
        if (hg && hg->type == JType::Object) {
            const JNode *f = hg->get("Field");
            int64_t sv = 0;
            uint64_t uv = 0;
            if (!f || f->type != JType::String || f->text.empty() || f->text.size() > BSG_MINMAX_MAX_NAME) return BSE_E_INVALID_QUERY;
            q.hist.field = f->text;
            if (!integer_member(hg->get("Origin"), true, sv, uv)) return BSE_E_INVALID_QUERY;
            q.hist.origin = sv;
            if (!integer_member(hg->get("Width"), false, sv, uv) || uv == 0) return BSE_E_INVALID_QUERY;
            q.hist.width = uv;
            if (!integer_member(hg->get("Buckets"), false, sv, uv) || uv == 0 || uv > BSG_HIST_MAX_BUCKETS) return BSE_E_INVALID_QUERY;
            q.hist.buckets = (uint32_t)uv;
            q.has_hist = true;
        } else if (hg && hg->type != JType::Null) {
            return BSE_E_INVALID_QUERY;
        }
        // "Prefilter": {"Expression": tree} in the reference's shape (QueryPrefilter); a nil Expression prunes nothing
        const JNode *pf = dom.get("Prefilter");
        if (pf && pf->type == JType::Object) {
            const JNode *ex = pf->get("Expression");
            if (ex && ex->type == JType::Object) {
                if (!prefilter_from_json(*ex, q.prefilter)) return BSE_E_INVALID_QUERY;
                q.has_prefilter = true;
            }
        } else if (pf && pf->type != JType::Null) {
            return BSE_E_INVALID_QUERY;
        }
    } else if (dom.type != JType::Null) {
        return BSE_E_INVALID_QUERY;
    }
    return 0;
}

// A "Histogram" query's counts.  The device route (query_many under DeviceMatchHistogram) has them in res.hist; on the host route the
// engine has matched as for any query and every matching row is bucketed here by hist_row_slot (what bsh_hist_row answers; a row that is
// no JSON object counts as missing).  Either way the result carries "rows": [] and the counts.
void histogram_to_json(const QueryResult &res, const ParsedQuery &q, std::string &out)
{
    const uint32_t B = q.hist.buckets;
    std::vector<uint64_t> counts = res.hist;
    if (counts.size() != (size_t)B + 3) {
        counts.assign((size_t)B + 3, 0);
        for (const std::string &row : res.rows) {
            uint32_t slot = B + 2u;
            if (!hist_row_slot(row, q.hist.field, q.hist.origin, q.hist.width, B, slot)) slot = B + 2u;
            ++counts[slot];
        }
    }
    out += "\"Histogram\":{\"Counts\":[";
    for (uint32_t b = 0; b < B; ++b) { if (b) out.push_back(','); out += std::to_string(counts[b]); }
    out += "],\"Below\":" + std::to_string(counts[B]) + ",\"Above\":" + std::to_string(counts[B + 1u]) + ",\"Missing\":" + std::to_string(counts[B + 2u]) + "},";
}

void result_to_json(const QueryResult &res, std::string &out, const ParsedQuery *q = nullptr)
{
    const bool hist = q && q->has_hist;
    out += "{\"rows\":[";
    for (size_t i = 0; i < res.rows.size() && !hist; ++i) { if (i) out.push_back(','); out += res.rows[i]; }
    out += "],";
    if (hist) histogram_to_json(res, *q, out);
    out += "\"stats\":{\"BlockStats\":[";
    for (size_t i = 0; i < res.block_stats.size(); ++i) {
        const BlockStats &s = res.block_stats[i];
        if (i) out.push_back(',');
        out += "{\"FileID\":" + std::to_string(s.file_id) + ",\"BlockOffset\":" + std::to_string(s.block_offset) +
               ",\"RowsProcessed\":" + std::to_string(s.rows_processed) + ",\"BytesProcessed\":" + std::to_string(s.bytes_processed) +
               ",\"TotalRows\":" + std::to_string(s.total_rows) + ",\"TotalBytes\":" + std::to_string(s.total_bytes) +
               ",\"Duration\":" + std::to_string(s.duration_ns) +
               ",\"BloomFilterSkipped\":" + (s.bloom_filter_skipped ? "true" : "false") + "}";
    }
    out += "],\"Errors\":[";
    for (size_t i = 0; i < res.errors.size(); ++i) { if (i) out.push_back(','); json_escape(out, res.errors[i]); }
    out += "],\"FilesConsidered\":" + std::to_string(res.files_considered) + ",\"FilesBloomSkipped\":" + std::to_string(res.files_bloom_skipped) + "}}";
}

}  // namespace

int32_t bse_query(bse_engine *e, const char *query_json, uint64_t len, char **out_json, uint64_t *out_len)
{
    if (!e || !out_json) return BSH_E_INVALID;
    ParsedQuery q;
    std::string_view sv(query_json ? query_json : "", query_json ? len : 0);
    if (!sv.empty()) {
        JNode dom;
        if (!parse_dom(sv, dom)) return BSE_E_INVALID_QUERY;
        if (int32_t rc = query_from_dom(dom, q)) return rc;
    }
    QueryResult res;
    if (int32_t rc = e->eng->query(q.nil ? nullptr : &q.expr, res, q.has_regex ? &q.regex : nullptr, q.has_sub ? &q.sub : nullptr, q.has_range ? &q.range : nullptr,
                                    q.has_prefilter ? &q.prefilter : nullptr)) return rc;
    std::string out;
    result_to_json(res, out, &q);
    return give(out, out_json, out_len);
}

int32_t bse_query_many(bse_engine *e, const char *queries_json, uint64_t len, char **out_json, uint64_t *out_len)
{
    if (!e || !out_json || !queries_json) return BSH_E_INVALID;
    JNode dom;
    if (!parse_dom(std::string_view(queries_json, len), dom) || dom.type != JType::Array) return BSE_E_INVALID_QUERY;
    std::vector<ParsedQuery> qs(dom.items.size());
    for (size_t i = 0; i < qs.size(); ++i)
        if (int32_t rc = query_from_dom(dom.items[i], qs[i])) return rc;
    std::vector<const BloomExpression *> exprs;
    std::vector<const RegexExpression *> regexes;
    std::vector<const SubstringExpression *> subs;
    std::vector<const RangeExpression *> ranges;
    std::vector<const PrefilterExpression *> prefilters;
    std::vector<const HistSpec *> hists;
    for (const ParsedQuery &q : qs) {
        hists.push_back(q.has_hist ? &q.hist : nullptr);
        prefilters.push_back(q.has_prefilter ? &q.prefilter : nullptr);
        exprs.push_back(q.nil ? nullptr : &q.expr); regexes.push_back(q.has_regex ? &q.regex : nullptr); subs.push_back(q.has_sub ? &q.sub : nullptr);
        ranges.push_back(q.has_range ? &q.range : nullptr);
    }
    std::vector<QueryResult> res;
    if (int32_t rc = e->eng->query_many(exprs, regexes, res, &subs, &ranges, &prefilters, &hists)) return rc;
    std::string out = "[";
    for (size_t i = 0; i < res.size(); ++i) { if (i) out.push_back(','); result_to_json(res[i], out, &qs[i]); }
    out.push_back(']');
    return give(out, out_json, out_len);
}

// {"<entry point>": calls, ...}: the device row-matcher entry points the engine has called since bse_open
int32_t bse_match_calls(bse_engine *e, char **out_json, uint64_t *out_len)
{
    if (!e || !out_json) return BSH_E_INVALID;
    std::string out = "{";
    for (const auto &kv : e->eng->match_calls()) {
        if (out.size() > 1) out.push_back(',');
        out += "\"" + kv.first + "\":" + std::to_string(kv.second);
    }
    out.push_back('}');
    return give(out, out_json, out_len);
}

int32_t bse_describe(bse_engine *e, char **out_json, uint64_t *out_len)
{
    if (!e || !out_json) return BSH_E_INVALID;
    auto counts = [](const BloomEntryCounts &c) {
        return "{\"Fields\":" + std::to_string(c.fields) + ",\"Tokens\":" + std::to_string(c.tokens) + ",\"FieldTokens\":" + std::to_string(c.field_tokens) + "}";
    };
    auto filters = [](const std::vector<uint8_t> &sec) {
        ParsedFilter pf[3];
        std::string s = "[";
        if (parse_filter_section(sec.data(), sec.size(), pf) == 0)
            for (int c = 0; c < 3; ++c) {
                if (c) s.push_back(',');
                s += pf[c].present ? "{\"m\":" + std::to_string(pf[c].m) + ",\"k\":" + std::to_string(pf[c].k) + "}" : "null";
            }
        return s + "]";
    };
    std::string out = "{\"files\":[";
    bool first_f = true;
    for (const DataFile &f : e->eng->files()) {
        if (!first_f) out.push_back(',');
        first_f = false;
        out += "{\"FileID\":" + std::to_string(f.file_id) + ",\"BloomEntryCounts\":" + counts(f.counts) +
               ",\"BloomFilterSize\":" + std::to_string(f.filter_section.size()) + ",\"filters\":" + filters(f.filter_section) + ",\"blocks\":[";
        for (size_t b = 0; b < f.blocks.size(); ++b) {
            const DataBlock &blk = f.blocks[b];
            if (b) out.push_back(',');
            out += "{\"PartitionID\":";
            json_escape(out, blk.partition_id);
            out += ",\"Rows\":" + std::to_string(blk.rows.size()) + ",\"BlockOffset\":" + std::to_string(blk.block_offset) +
                   ",\"BloomEntryCounts\":" + counts(blk.counts) + ",\"BloomFalsePositiveRate\":" + std::to_string(blk.fpr) +
                   ",\"BloomFilterSize\":" + std::to_string(blk.filter_section.size()) + ",\"filters\":" + filters(blk.filter_section);
            if (!blk.minmax.empty()) {             // DataBlockMetadata.MinMaxIndexes (omitempty)
                out += ",\"MinMaxIndexes\":{";
                bool first_i = true;
                for (const auto &kv : blk.minmax) {
                    if (!first_i) out.push_back(',');
                    first_i = false;
                    json_escape(out, kv.first);
                    out += ":{\"Min\":" + std::to_string(kv.second.min) + ",\"Max\":" + std::to_string(kv.second.max) + "}";
                }
                out.push_back('}');
            }
            out.push_back('}');
        }
        out += "]}";
    }
    const BloomSearchEngine::StreamStats &ss = e->eng->stream_stats();
    out += "],\"IngestStream\":{\"Batches\":" + std::to_string(ss.batches) + ",\"Rows\":" + std::to_string(ss.rows) +
           ",\"HostRows\":" + std::to_string(ss.host_rows) + ",\"Flushes\":" + std::to_string(ss.flushes) + "}}";
    return give(out, out_json, out_len);
}

int32_t bse_corrupt_section_byte(bse_engine *e, uint32_t file_index, int32_t block_index, uint64_t byte_index)
{
    if (!e) return BSH_E_INVALID;
    return e->eng->corrupt_section_byte(file_index, block_index, byte_index) ? 0 : BSH_E_INVALID;
}

int32_t bse_section_bytes(bse_engine *e, uint32_t file_index, int32_t block_index, uint8_t **out, uint64_t *out_len)
{
    if (!e || !out || !out_len) return BSH_E_INVALID;
    const auto &files = e->eng->files();
    if (file_index >= files.size()) return BSH_E_INVALID;
    const std::vector<uint8_t> *sec = &files[file_index].filter_section;
    if (block_index >= 0) {
        if ((size_t)block_index >= files[file_index].blocks.size()) return BSH_E_INVALID;
        sec = &files[file_index].blocks[block_index].filter_section;
    }
    uint8_t *p = static_cast<uint8_t *>(malloc(std::max<size_t>(sec->size(), 1)));
    memcpy(p, sec->data(), sec->size());
    *out = p;
    *out_len = sec->size();
    return 0;
}

}  // extern "C"
