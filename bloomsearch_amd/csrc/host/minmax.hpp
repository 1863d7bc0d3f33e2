// minmax.hpp — per-block MinMax indexes on the host (the mirror of csrc/minmax.hip.h; contract: include/bloomgpu.h "MinMax indexes").
//   * minmax_of_literal: a JSON number literal -> (clamp(floor(v)), clamp(ceil(v))) from range.hpp's normal form (sign, digit string,
//     point position).  Exact for EVERY literal, exponents of any size included; no floating point.
//   * minmax_row: one row's contributions folded into an index per field.  Fields are top-level keys compared byte for byte with the
//     DECODED key; the last member with the key counts; its value must itself be a number.
//   * minmax_eval: EvaluateMinMaxCondition's ten operators (query.go), with the saturation rules at the int64 extremes.
//   * PrefilterExpression / prefilter_eval: CONDITION | AND | OR over PARTITION and MINMAX conditions as evaluatePrefilterExpression:
//     an empty Or is false, an empty And true, a nil condition true, a block without the named index FALSE, an empty partition id
//     fails every partition condition, an unknown node or operator is false.
// Host-only (plain g++), like arena_cache.hpp and range_groups.hpp.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <string_view>
#include <vector>

#include "bloomgpu.h"
#include "json.hpp"
#include "range.hpp"

namespace bsh {

enum MinMaxOp : uint32_t { MM_EQ = 0, MM_NE, MM_GT, MM_GE, MM_LT, MM_LE, MM_IN, MM_NOT_IN, MM_BETWEEN, MM_NOT_BETWEEN, MM_OP_COUNT };

// UpdateMinMaxIndex: the fold of one contribution into an index
inline void minmax_fold(bsg_minmax &idx, int64_t mn, int64_t mx)
{
    if (!idx.present) { idx.min = mn; idx.max = mx; idx.present = 1; return; }
    if (mn < idx.min) idx.min = mn;
    if (mx > idx.max) idx.max = mx;
}

// floor and ceil of the literal's exact value, clamped to int64.  false: not a number literal.
inline bool minmax_of_literal(std::string_view literal, int64_t &mn, int64_t &mx)
{
    DecimalLiteral v;
    if (!parse_decimal_literal(literal, v)) return false;
    if (v.digits.empty()) { mn = mx = 0; return true; }            // 0, -0, -0.0, 0e5
    const bool neg = v.neg;
    uint64_t mag = 0;                                               // the integer part of |v|, where it can matter
    bool frac = true, huge = false;
    if (v.point <= 0) mag = 0;                                      // 0 < |v| < 1
    else if (v.point > 19) huge = true;                             // |v| >= 10^19 > 2^63
    else {
        const size_t n = v.digits.size(), ip = (size_t)v.point;
        for (size_t i = 0; i < ip; ++i) mag = mag * 10 + (uint64_t)(i < n ? v.digits[i] - '0' : 0);   // <= 19 digits: no wrap
        frac = n > ip;                                              // the digit string ends in a non-zero digit
    }
    const uint64_t lim = uint64_t(1) << 63;
    if (!neg) {
        if (huge || mag > lim - 1) { mn = mx = INT64_MAX; return true; }
        mn = (int64_t)mag;
        mx = (frac && mag == lim - 1) ? INT64_MAX : (int64_t)(mag + (frac ? 1 : 0));
    } else {
        if (huge || mag > lim) { mn = mx = INT64_MIN; return true; }
        mx = mag == lim ? INT64_MIN : -(int64_t)mag;               // ceil(-(mag + f)) = -mag
        const uint64_t down = mag + (frac ? 1 : 0);
        mn = down >= lim ? INT64_MIN : -(int64_t)down;
    }
    return true;
}

struct MinMaxFieldNames {
    std::vector<std::string> names;
    // 1 to BSG_MINMAX_MAX_FIELDS distinct names of 1 to BSG_MINMAX_MAX_NAME bytes; on failure `why` names the field
    static bool check(const std::vector<std::string> &names, std::string &why)
    {
        if (names.empty() || names.size() > BSG_MINMAX_MAX_FIELDS) { why = "between 1 and 8 fields"; return false; }
        for (size_t f = 0; f < names.size(); ++f) {
            if (names[f].empty()) { why = "field " + std::to_string(f) + " has an empty name"; return false; }
            if (names[f].size() > BSG_MINMAX_MAX_NAME) { why = "the name of field " + std::to_string(f) + " is longer than 64 bytes"; return false; }
            for (size_t g = 0; g < f; ++g)
                if (names[g] == names[f]) { why = "fields " + std::to_string(g) + " and " + std::to_string(f) + " have the same name"; return false; }
        }
        return true;
    }
    bool unpack(const uint8_t *bytes, const uint32_t *off, uint32_t n, std::string &why)
    {
        names.clear();
        if (!bytes || !off) { why = "null arrays"; return false; }
        if (n == 0 || n > BSG_MINMAX_MAX_FIELDS) { why = "between 1 and 8 fields"; return false; }
        for (uint32_t f = 0; f < n; ++f) {
            if (off[f + 1] < off[f]) { why = "offsets not monotone"; return false; }
            names.emplace_back((const char *)bytes + off[f], off[f + 1] - off[f]);
        }
        return check(names, why);
    }
};

// One row's contributions folded into inout[n_fields].  false: the row is not one valid JSON object (nothing is folded).
inline bool minmax_row(std::string_view row, const std::vector<std::string> &fields, bsg_minmax *inout)
{
    const size_t nf = fields.size();
    std::vector<uint8_t> have(nf, 0);
    std::vector<int64_t> mn(nf, 0), mx(nf, 0);
    JScanner sc(row.data(), row.size());
    std::string key, scratch;
    sc.skip_ws();
    if (sc.p >= sc.end || *sc.p != '{') return false;
    ++sc.p;
    sc.skip_ws();
    if (sc.p < sc.end && *sc.p == '}') ++sc.p;
    else {
        for (;;) {
            sc.skip_ws();
            key.clear();
            if (!sc.parse_string(key)) return false;
            sc.skip_ws();
            if (sc.p >= sc.end || *sc.p != ':') return false;
            ++sc.p;
            sc.skip_ws();
            const char *v0 = sc.p;
            const char c = sc.p < sc.end ? *sc.p : 0;
            if (!validate_value(sc, scratch, 1)) return false;
            for (size_t f = 0; f < nf; ++f) {
                if (fields[f] != key) continue;
                have[f] = 0;                                        // the last member with the key counts, number or not
                if (c == '-' || (c >= '0' && c <= '9')) have[f] = minmax_of_literal(std::string_view(v0, (size_t)(sc.p - v0)), mn[f], mx[f]) ? 1 : 0;
            }
            sc.skip_ws();
            if (sc.p < sc.end && *sc.p == ',') { ++sc.p; continue; }
            if (sc.p < sc.end && *sc.p == '}') { ++sc.p; break; }
            return false;
        }
    }
    sc.skip_ws();
    if (!sc.ok || sc.p != sc.end) return false;
    for (size_t f = 0; f < nf; ++f) if (have[f]) minmax_fold(inout[f], mn[f], mx[f]);
    return true;
}

// One row's slot among the n_buckets + 3 of a bucketed hit count (bloomgpu.h "Bucketed hit counts"): t = the `min` half of the row's
// contribution to `field`; t < origin is below (slot B), else q = ((uint64)t - (uint64)origin) / width, bucket q or above (B + 1);
// a row without a number on the field's last member is missing (B + 2).  width >= 1.  false: the row is not one valid JSON object.
inline bool hist_row_slot(std::string_view row, const std::string &field, int64_t origin, uint64_t width, uint32_t n_buckets, uint32_t &slot)
{
    bsg_minmax idx{};
    if (!minmax_row(row, std::vector<std::string>{field}, &idx)) return false;
    if (!idx.present) slot = n_buckets + 2u;
    else if (idx.min < origin) slot = n_buckets;
    else {
        const uint64_t q = ((uint64_t)idx.min - (uint64_t)origin) / width;
        slot = q >= (uint64_t)n_buckets ? n_buckets + 1u : (uint32_t)q;
    }
    return true;
}

// EvaluateMinMaxCondition.  A bound stored at an int64 extreme is saturated: the true value may lie beyond it, so an operator whose
// strict comparison at that boundary would drop the block keeps it.  NOT_IN is always true; an unknown operator false.
inline bool minmax_eval(int64_t imin, int64_t imax, uint32_t op, int64_t value, const int64_t *values, size_t n_values, int64_t lo, int64_t hi)
{
    const bool sat_above = imax == INT64_MAX, sat_below = imin == INT64_MIN;
    switch (op) {
    case MM_EQ: return imin <= value && value <= imax;
    case MM_NE: return imin != value || imax != value || sat_above || sat_below;
    case MM_GT: return imax > value || sat_above;
    case MM_GE: return imax >= value;
    case MM_LT: return imin < value || sat_below;
    case MM_LE: return imin <= value;
    case MM_IN:
        for (size_t i = 0; i < n_values; ++i) if (imin <= values[i] && values[i] <= imax) return true;
        return false;
    case MM_NOT_IN: return true;
    case MM_BETWEEN: return imin <= hi && lo <= imax;
    case MM_NOT_BETWEEN: return imin < lo || imax > hi || sat_above || sat_below;
    default: return false;
    }
}

// EvaluateStringCondition with the same operator numbering (byte-wise comparison, as Go compares strings)
inline bool string_condition_eval(std::string_view v, uint32_t op, std::string_view value, const std::vector<std::string> &values, std::string_view lo,
                                  std::string_view hi)
{
    switch (op) {
    case MM_EQ: return v == value;
    case MM_NE: return v != value;
    case MM_GT: return v > value;
    case MM_GE: return v >= value;
    case MM_LT: return v < value;
    case MM_LE: return v <= value;
    case MM_IN:
        for (auto &x : values) if (v == x) return true;
        return false;
    case MM_NOT_IN:
        for (auto &x : values) if (v == x) return false;
        return true;
    case MM_BETWEEN: return v >= lo && v <= hi;
    case MM_NOT_BETWEEN: return v < lo || v > hi;
    default: return false;
    }
}

// ---- the prefilter tree ----
enum class PrefilterType : uint8_t { Unknown, Condition, And, Or };
enum class PrefilterKind : uint8_t { Unknown, Partition, MinMax };

struct PrefilterExpression {
    PrefilterType type = PrefilterType::Unknown;
    bool has_condition = false;               // "Condition" is an object
    PrefilterKind kind = PrefilterKind::Unknown;
    bool has_operand = false;                 // the PartitionCondition / MinMaxCondition of the kind is an object (nil: always true)
    std::string field;                        // MinMaxFieldName
    uint32_t op = MM_OP_COUNT;
    int64_t value = 0, lo = 0, hi = 0;        // MinMax: Value, Min, Max
    std::vector<int64_t> values;
    std::string svalue, slo, shi;             // Partition: Value, Min, Max
    std::vector<std::string> svalues;
    std::vector<PrefilterExpression> children;
};

inline uint32_t minmax_op_from_name(std::string_view s)
{
    static const char *const names[MM_OP_COUNT] = {"EQ", "NE", "GT", "GTE", "LT", "LTE", "IN", "NOT_IN", "BETWEEN", "NOT_BETWEEN"};
    for (uint32_t i = 0; i < MM_OP_COUNT; ++i) if (s == names[i]) return i;
    return MM_OP_COUNT;
}

// What a block offers a prefilter
struct PrefilterBlock {
    std::string_view partition_id;
    const std::map<std::string, bsg_minmax> *indexes = nullptr;
};

inline bool prefilter_eval(const PrefilterExpression &e, const PrefilterBlock &b)
{
    switch (e.type) {
    case PrefilterType::Condition:
        if (!e.has_condition) return true;
        if (e.kind == PrefilterKind::Partition) {
            if (!e.has_operand) return true;
            if (b.partition_id.empty()) return false;
            return string_condition_eval(b.partition_id, e.op, e.svalue, e.svalues, e.slo, e.shi);
        }
        if (e.kind == PrefilterKind::MinMax) {
            if (!e.has_operand) return true;
            if (!b.indexes) return false;
            const auto it = b.indexes->find(e.field);
            if (it == b.indexes->end() || !it->second.present) return false;
            return minmax_eval(it->second.min, it->second.max, e.op, e.value, e.values.data(), e.values.size(), e.lo, e.hi);
        }
        return false;
    case PrefilterType::Or:
        for (auto &c : e.children) if (prefilter_eval(c, b)) return true;
        return false;
    case PrefilterType::And:
        for (auto &c : e.children) if (!prefilter_eval(c, b)) return false;
        return true;
    default:
        return false;
    }
}

// {"ExpressionType":"CONDITION"|"AND"|"OR","Condition":{"ConditionType":"PARTITION"|"MINMAX","PartitionCondition":{"Operator","Value",
// "Values","Min","Max"},"MinMaxFieldName","MinMaxCondition":{the same, int64}},"Children":[..]}.  false: a member of the wrong shape.
inline bool prefilter_from_json(const JNode &n, PrefilterExpression &out)
{
    if (n.type != JType::Object) return false;
    const JNode *t = n.get("ExpressionType");
    const std::string ts = (t && t->type == JType::String) ? t->text : "";
    out.type = ts == "CONDITION" ? PrefilterType::Condition : ts == "AND" ? PrefilterType::And : ts == "OR" ? PrefilterType::Or : PrefilterType::Unknown;
    const JNode *c = n.get("Condition");
    out.has_condition = c && c->type == JType::Object;
    if (out.has_condition) {
        const JNode *ct = c->get("ConditionType");
        const std::string cts = (ct && ct->type == JType::String) ? ct->text : "";
        out.kind = cts == "PARTITION" ? PrefilterKind::Partition : cts == "MINMAX" ? PrefilterKind::MinMax : PrefilterKind::Unknown;
        const JNode *f = c->get("MinMaxFieldName");
        out.field = (f && f->type == JType::String) ? f->text : "";
        const JNode *o = out.kind == PrefilterKind::Partition ? c->get("PartitionCondition") : out.kind == PrefilterKind::MinMax ? c->get("MinMaxCondition") : nullptr;
        out.has_operand = o && o->type == JType::Object;
        if (out.has_operand) {
            const JNode *op = o->get("Operator"), *v = o->get("Value"), *vs = o->get("Values"), *lo = o->get("Min"), *hi = o->get("Max");
            out.op = (op && op->type == JType::String) ? minmax_op_from_name(op->text) : (uint32_t)MM_OP_COUNT;
            const bool num = out.kind == PrefilterKind::MinMax;
            auto scalar = [&](const JNode *x, int64_t &i, std::string &s) {
                if (!x || x->type == JType::Null) return true;
                if (num) return int64_from_json(*x, i);
                if (x->type != JType::String) return false;
                s = x->text;
                return true;
            };
            if (!scalar(v, out.value, out.svalue) || !scalar(lo, out.lo, out.slo) || !scalar(hi, out.hi, out.shi)) return false;
            if (vs && vs->type == JType::Array)
                for (const JNode &x : vs->items) {
                    int64_t i = 0;
                    std::string s;
                    if (!scalar(&x, i, s)) return false;
                    if (num) out.values.push_back(i); else out.svalues.push_back(std::move(s));
                }
        }
    }
    const JNode *kids = n.get("Children");
    if (kids && kids->type == JType::Array) {
        out.children.resize(kids->items.size());
        for (size_t i = 0; i < kids->items.size(); ++i)
            if (!prefilter_from_json(kids->items[i], out.children[i])) return false;
    }
    return true;
}

}  // namespace bsh
