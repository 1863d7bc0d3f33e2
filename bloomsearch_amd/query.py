"""Bloom query algebra: a host-side mirror of the reference's BloomExpression tree.

Mirrors query.go:478-610 (BloomCondition / BloomExpression, Field / Token /
FieldToken / And / Or with same-type flattening, flattenExpressions :600-610)
and AndBloomQueries (:709-718).  Expressions are plain dicts in the exact JSON
shape of the reference's exported structs, so a tree serialised by a Go
MetaStore/tool loads unchanged.

compile_queries() lowers a batch of trees to the C-ABI form (bloomgpu.h):
distinct terms (the probed strings + filter kind) and one postfix program per
query, following evaluateBloomExpression / evaluateBloomCondition
(query_exec.go:89-159) case by case.
"""
from __future__ import annotations

import numpy as np

from ._lib import RANGE_HI_OPEN, RANGE_LO_OPEN, RANGE_NO_HI, RANGE_NO_LO, KIND_FIELD, KIND_FIELD_RANGE, KIND_FIELD_REGEX, KIND_FIELD_SUBSTRING, KIND_FIELD_TOKEN, KIND_SUBSTRING, KIND_TOKEN, OP_AND, OP_FALSE, OP_OR, OP_TERM, OP_TRUE, op

BLOOM_FIELD, BLOOM_TOKEN, BLOOM_FIELD_TOKEN = "FIELD", "TOKEN", "FIELD_TOKEN"
EXPR_CONDITION, EXPR_AND, EXPR_OR = "CONDITION", "AND", "OR"


def Field(field: str) -> dict:
    return {"ExpressionType": EXPR_CONDITION, "Condition": {"Type": BLOOM_FIELD, "Field": field, "Token": ""}}


def Token(token: str) -> dict:
    return {"ExpressionType": EXPR_CONDITION, "Condition": {"Type": BLOOM_TOKEN, "Field": "", "Token": token}}


def FieldToken(field: str, token: str) -> dict:
    return {"ExpressionType": EXPR_CONDITION,
            "Condition": {"Type": BLOOM_FIELD_TOKEN, "Field": field, "Token": token}}


def _flatten(expressions, expression_type):
    # query.go:600-610: a child of the same type with no Condition is spliced in
    out = []
    for e in expressions:
        if e.get("ExpressionType") == expression_type and e.get("Condition") is None:
            out.extend(e.get("Children") or [])
        else:
            out.append(e)
    return out


def And(*expressions) -> dict:
    return {"ExpressionType": EXPR_AND, "Children": _flatten(expressions, EXPR_AND)}


def Or(*expressions) -> dict:
    return {"ExpressionType": EXPR_OR, "Children": _flatten(expressions, EXPR_OR)}


def and_bloom_queries(left, right):
    """AndBloomQueries (query.go:709-718) on bare expressions (None == nil query)."""
    if left is None:
        return right
    if right is None:
        return left
    return And(left, right)


# ---- regex query tree (query.go:520-538, :612-649) and its bloom field guard (:651-707) ----
def FieldRegex(field: str, pattern: str) -> dict:
    return {"ExpressionType": "CONDITION", "Condition": {"Field": field, "Pattern": pattern}}


def _flatten_regex(expressions, expression_type):
    out = []
    for e in expressions:
        if e.get("ExpressionType") == expression_type and e.get("Condition") is None:
            out.extend(e.get("Children") or [])
        else:
            out.append(e)
    return out


def RegexAnd(*expressions) -> dict:
    return {"ExpressionType": "AND", "Children": _flatten_regex(expressions, "AND")}


def RegexOr(*expressions) -> dict:
    return {"ExpressionType": "OR", "Children": _flatten_regex(expressions, "OR")}


def regex_field_guard_bloom_query(regex_expression):
    """RegexFieldGuardBloomQuery (query.go:698-707) on bare expressions: every regex condition becomes Field(cond.Field);
    And / Or keep their node around whatever children translate (no flattening); anything else is nil."""
    if regex_expression is None:
        return None
    t = regex_expression.get("ExpressionType")
    if t == "CONDITION":
        c = regex_expression.get("Condition")
        return None if c is None else Field(c.get("Field", ""))
    if t in ("AND", "OR"):
        kids = [g for g in (regex_field_guard_bloom_query(c) for c in regex_expression.get("Children") or []) if g is not None]
        return {"ExpressionType": EXPR_AND if t == "AND" else EXPR_OR, "Children": kids}
    return None


# ---- substring query tree and its bloom guard (bloomgpu.h "Substring conditions"; host/substring.hpp is the implementation) ----
def Substring(needle: str) -> dict:
    """Some leaf's text contains the needle (folded as the store's tokenizer folds)."""
    return {"ExpressionType": "CONDITION", "Condition": {"Needle": needle}}


def FieldSubstring(field: str, needle: str) -> dict:
    """... a leaf whose path equals `field`."""
    return {"ExpressionType": "CONDITION", "Condition": {"Field": field, "Needle": needle}}


def SubstringAnd(*expressions) -> dict:
    return {"ExpressionType": "AND", "Children": _flatten_regex(expressions, "AND")}


def SubstringOr(*expressions) -> dict:
    return {"ExpressionType": "OR", "Children": _flatten_regex(expressions, "OR")}


NIL_CONDITION = {"ExpressionType": EXPR_CONDITION, "Condition": None}       # always true (query_exec.go:101-104)


def substring_terms(needle, tokenizer=None) -> list:
    """The tokens a row that contains `needle` must hold under `tokenizer` (None = the default), through the library
    (bsh_substring_terms): deduplicated, in first-occurrence order."""
    from . import host
    return host.substring_terms(needle, tokenizer)


def substring_guard_bloom_query(substring_expression, tokenizer=None):
    """The tree as a bloom expression over its pruning terms: a condition is And(Token(t) ..) / And(FieldToken(field, t) ..); without
    terms Field(field), or for an any-field condition nil (always true), which an And drops and an Or keeps as NIL_CONDITION.
    None = nil."""
    e = substring_expression
    if e is None:
        return None
    t = e.get("ExpressionType")
    if t == "CONDITION":
        c = e.get("Condition")
        if c is None:
            return None
        field, terms = c.get("Field"), substring_terms(c.get("Needle", ""), tokenizer)
        if not terms:
            return None if field is None else Field(field)
        return And(*[Token(w) if field is None else FieldToken(field, w) for w in terms])
    if t in ("AND", "OR"):
        kids = [substring_guard_bloom_query(c, tokenizer) for c in e.get("Children") or []]
        if t == "AND":
            kept = [k for k in kids if k is not None]
            return None if kids and not kept else {"ExpressionType": EXPR_AND, "Children": kept}
        return {"ExpressionType": EXPR_OR, "Children": [NIL_CONDITION if k is None else k for k in kids]}
    return None


def prune_bloom_query(bloom_expression, regex_expression, substring_expression=None, tokenizer=None):
    """pruneBloomQuery (query_exec.go:220), with the substring tree's guard as a third side."""
    two = and_bloom_queries(bloom_expression, regex_field_guard_bloom_query(regex_expression))
    return and_bloom_queries(two, substring_guard_bloom_query(substring_expression, tokenizer))


# ---- range query tree and its bloom guard (bloomgpu.h "Range conditions"; host/range.hpp is the implementation) ----
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def FieldRange(field: str, lo=None, hi=None, lo_open: bool = False, hi_open: bool = False) -> dict:
    """Some NUMBER leaf whose path equals `field` has a value inside the interval: int64 bounds, None = unbounded, each closed
    unless lo_open / hi_open.  The value is the literal's exact decimal value."""
    for b in (lo, hi):
        if b is not None and not (isinstance(b, int) and not isinstance(b, bool) and INT64_MIN <= b <= INT64_MAX):
            raise ValueError(f"range bound {b!r}: an int64 or None")
    c = {"Field": field}
    if lo is not None:
        c["Lo"] = lo
    if hi is not None:
        c["Hi"] = hi
    if lo_open:
        c["LoOpen"] = True
    if hi_open:
        c["HiOpen"] = True
    return {"ExpressionType": "CONDITION", "Condition": c}


def RangeAnd(*expressions) -> dict:
    return {"ExpressionType": "AND", "Children": _flatten_regex(expressions, "AND")}


def RangeOr(*expressions) -> dict:
    return {"ExpressionType": "OR", "Children": _flatten_regex(expressions, "OR")}


def numeric_condition_range(field: str, condition: dict) -> dict:
    """The reference's NumericCondition ({"Operator", "Value" | "Values" | "Min", "Max"}, query.go:37-44) as a range tree over the
    number leaves of `field`: EQ, GT, GTE, LT, LTE and BETWEEN are one interval; NE and NOT_BETWEEN the Or of the two outside
    intervals; IN an Or of points; NOT_IN the Or of the gaps between the sorted points (open at both points, so 5.5 lies in the gap
    between 5 and 6).  The tree holds when SOME leaf's value satisfies the operator."""
    o = condition.get("Operator")
    v, lo, hi = condition.get("Value", 0), condition.get("Min", 0), condition.get("Max", 0)
    if o == "EQ":
        return FieldRange(field, v, v)
    if o == "GT":
        return FieldRange(field, v, None, lo_open=True)
    if o == "GTE":
        return FieldRange(field, v, None)
    if o == "LT":
        return FieldRange(field, None, v, hi_open=True)
    if o == "LTE":
        return FieldRange(field, None, v)
    if o == "BETWEEN":
        return FieldRange(field, lo, hi)
    if o == "NE":
        return RangeOr(FieldRange(field, None, v, hi_open=True), FieldRange(field, v, None, lo_open=True))
    if o == "NOT_BETWEEN":
        return RangeOr(FieldRange(field, None, lo, hi_open=True), FieldRange(field, hi, None, lo_open=True))
    if o == "IN":
        return RangeOr(*[FieldRange(field, p, p) for p in condition.get("Values") or []])
    if o == "NOT_IN":
        pts = sorted(set(condition.get("Values") or []))
        edges = [None] + pts + [None]
        return RangeOr(*[FieldRange(field, a, b, lo_open=a is not None, hi_open=b is not None) for a, b in zip(edges, edges[1:])])
    raise ValueError(f"numeric operator {o!r}")


# ---- prefilter tree over block metadata (query.go PrefilterExpression): partition ids and MinMax indexes ----
PREFILTER_OPS = ("EQ", "NE", "GT", "GTE", "LT", "LTE", "IN", "NOT_IN", "BETWEEN", "NOT_BETWEEN")


def _prefilter_condition(op: str, operands, check) -> dict:
    """{"Operator", "Value" | "Values" | "Min", "Max"} as the reference's StringCondition / NumericCondition"""
    if op not in PREFILTER_OPS:
        raise ValueError(f"prefilter operator {op!r}")
    for v in operands:
        check(v)
    if op in ("IN", "NOT_IN"):
        return {"Operator": op, "Values": list(operands)}
    if op in ("BETWEEN", "NOT_BETWEEN"):
        lo, hi = operands
        return {"Operator": op, "Min": lo, "Max": hi}
    (v,) = operands
    return {"Operator": op, "Value": v}


def _check_int64(v):
    if not (isinstance(v, int) and not isinstance(v, bool) and INT64_MIN <= v <= INT64_MAX):
        raise ValueError(f"MinMax operand {v!r}: an int64")


def _check_str(v):
    if not isinstance(v, str):
        raise ValueError(f"partition operand {v!r}: a string")


def Partition(op: str, *operands) -> dict:
    """The block's partition id satisfies the operator: Partition("EQ", "p1"), Partition("IN", "a", "b"), Partition("BETWEEN", lo, hi).
    A block without a partition id fails every partition condition."""
    return {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "PARTITION", "PartitionCondition": _prefilter_condition(op, operands, _check_str)}}


def MinMax(field: str, op: str, *operands) -> dict:
    """The block's MinMax index of `field` (engine config "MinMaxIndexes") may hold a value that satisfies the operator:
    MinMax("ts", "GTE", 100), MinMax("ts", "BETWEEN", 0, 99), MinMax("ts", "IN", 1, 2, 3).  A block without the index fails."""
    return {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "MINMAX", "MinMaxFieldName": field,
                                                           "MinMaxCondition": _prefilter_condition(op, operands, _check_int64)}}


def PrefilterAnd(*expressions) -> dict:
    return {"ExpressionType": "AND", "Children": _flatten_regex(expressions, "AND")}


def PrefilterOr(*expressions) -> dict:
    return {"ExpressionType": "OR", "Children": _flatten_regex(expressions, "OR")}


def range_entry(condition: dict) -> bytes:
    """Entry 2i + 1 of a KIND_FIELD_RANGE condition: lo, hi (int64, little-endian) and the flag byte."""
    lo, hi = condition.get("Lo"), condition.get("Hi")
    flags = (RANGE_NO_LO if lo is None else 0) | (RANGE_NO_HI if hi is None else 0) | \
            (RANGE_LO_OPEN if condition.get("LoOpen") else 0) | (RANGE_HI_OPEN if condition.get("HiOpen") else 0)
    return (lo or 0).to_bytes(8, "little", signed=True) + (hi or 0).to_bytes(8, "little", signed=True) + bytes([flags])


def range_guard_bloom_query(range_expression):
    """The tree with every condition as Field(field); the nil condition is dropped from an And and kept in an Or (NIL_CONDITION), as
    in the substring guard.  None = nil."""
    e = range_expression
    if e is None:
        return None
    t = e.get("ExpressionType")
    if t == "CONDITION":
        c = e.get("Condition")
        return None if c is None else Field(c.get("Field", ""))
    if t in ("AND", "OR"):
        kids = [range_guard_bloom_query(c) for c in e.get("Children") or []]
        if t == "AND":
            kept = [k for k in kids if k is not None]
            return None if kids and not kept else {"ExpressionType": EXPR_AND, "Children": kept}
        return {"ExpressionType": EXPR_OR, "Children": [NIL_CONDITION if k is None else k for k in kids]}
    return None


def make_field_token_key(field: str, token: str) -> str:
    """makeFieldTokenKey (tokenizer.go:509-511): plain concatenation, no escaping."""
    return field + "::" + token


def term_of(condition: dict):
    """(kind, probed string) for a known condition type, else None (query_exec.go:134-157)."""
    t = condition.get("Type")
    if t == BLOOM_FIELD:
        return KIND_FIELD, condition.get("Field", "")
    if t == BLOOM_TOKEN:
        return KIND_TOKEN, condition.get("Token", "")
    if t == BLOOM_FIELD_TOKEN:
        return KIND_FIELD_TOKEN, make_field_token_key(condition.get("Field", ""), condition.get("Token", ""))
    return None


class CompiledBatch:
    """Distinct terms + per-query postfix programs for a batch of queries."""

    def __init__(self):
        self.term_strings: list[bytes] = []
        self.term_kinds: list[int] = []
        self._index: dict = {}
        self.prog_ops: list[int] = []
        self.prog_off: list[int] = [0]

    def _term(self, kind: int, s: str) -> int:
        key = (kind, s)
        i = self._index.get(key)
        if i is None:
            i = len(self.term_strings)
            self._index[key] = i
            self.term_strings.append(s.encode("utf-8", "surrogatepass"))
            self.term_kinds.append(kind)
        return i

    def _emit(self, e) -> None:
        if e is None:                       # nil expression => true (query_exec.go:96-98)
            self.prog_ops.append(op(OP_TRUE))
            return
        et = e.get("ExpressionType")
        if et == EXPR_CONDITION:
            cond = e.get("Condition")
            if cond is None:                # nil condition => true (:101-104)
                self.prog_ops.append(op(OP_TRUE))
                return
            t = term_of(cond)
            if t is None:                   # unknown condition type => false (:155-156)
                self.prog_ops.append(op(OP_FALSE))
            else:
                self.prog_ops.append(op(OP_TERM, self._term(*t)))
        elif et in (EXPR_AND, EXPR_OR):
            kids = e.get("Children") or []
            for c in kids:
                self._emit(c)
            self.prog_ops.append(op(OP_AND if et == EXPR_AND else OP_OR, len(kids)))
        else:                               # unknown expression type => false (:122-123)
            self.prog_ops.append(op(OP_FALSE))

    def add_query(self, expression) -> None:
        """expression None == nil BloomQuery / nil Expression => no ops => true (:81-83)."""
        if expression is not None:
            self._emit(expression)
        self.prog_off.append(len(self.prog_ops))

    @property
    def n_queries(self) -> int:
        return len(self.prog_off) - 1

    def arrays(self):
        return (np.asarray(self.prog_ops, dtype=np.uint32), np.asarray(self.prog_off, dtype=np.uint32),
                np.asarray(self.term_kinds, dtype=np.uint32))


def compile_queries(expressions) -> CompiledBatch:
    cb = CompiledBatch()
    for e in expressions:
        cb.add_query(e)
    return cb


class CompiledMatcher:
    """One expression for the device row matcher (include/bloomgpu.h bsg_match_rows): its conditions — field and token
    strings kept APART, because FieldToken is a (path, token) pair at one leaf, not the joined bloom key
    (row_matcher.go:587) — and the postfix program over condition indices."""

    def __init__(self, expression):
        self.kinds: list[int] = []
        self.fields: list[bytes] = []
        self.tokens: list[bytes] = []
        self.prog_ops: list[int] = []
        if expression is not None:
            self._emit(expression)

    def _emit(self, e) -> None:
        if e is None:
            self.prog_ops.append(op(OP_TRUE))
            return
        et = e.get("ExpressionType")
        if et == EXPR_CONDITION:
            cond = e.get("Condition")
            if cond is None:                # nil condition => true (row_matcher.go:257-290)
                self.prog_ops.append(op(OP_TRUE))
                return
            t = cond.get("Type")
            if t not in (BLOOM_FIELD, BLOOM_TOKEN, BLOOM_FIELD_TOKEN):
                self.prog_ops.append(op(OP_FALSE))
                return
            self.prog_ops.append(op(OP_TERM, len(self.kinds)))
            self.kinds.append({BLOOM_FIELD: KIND_FIELD, BLOOM_TOKEN: KIND_TOKEN, BLOOM_FIELD_TOKEN: KIND_FIELD_TOKEN}[t])
            self.fields.append(cond.get("Field", "").encode("utf-8", "surrogatepass"))
            self.tokens.append(cond.get("Token", "").encode("utf-8", "surrogatepass"))
        elif et in (EXPR_AND, EXPR_OR):
            kids = e.get("Children") or []
            for c in kids:
                self._emit(c)
            self.prog_ops.append(op(OP_AND if et == EXPR_AND else OP_OR, len(kids)))
        else:
            self.prog_ops.append(op(OP_FALSE))


MATCH_MANY_MAX_QUERIES, MATCH_MANY_MAX_CONDS, MATCH_MANY_MAX_OPS = 64, 64, 2048      # bloomgpu.h bsg_match_rows_many
MATCH_MANY_MAX_REGEX_CONDS = 16                                                      # bloomgpu.h bsg_match_rows_many_regex


def lowered_ops(prog_ops) -> int:
    """Length of the binary program the library lowers a public postfix program to: an n-ary And / Or becomes n - 1 binary
    ops, an empty one a constant."""
    n = 0
    for o in prog_ops:
        opc, arg = o >> 28, o & 0x0FFFFFFF
        n += (arg - 1 if arg else 1) if opc in (OP_AND, OP_OR) else 1
    return n


class CompiledMatcherBatch:
    """A batch of expressions for one bsg_match_rows_many call: ONE table of distinct conditions — deduplicated across the
    queries by (kind, field, token) — and one postfix program per query over the table's indices (query q's is
    CompiledMatcher(expr_q)'s with its condition indices remapped).  Raises ValueError beyond the call's limits."""

    MAX_QUERIES, MAX_OPS, MAX_CONDS = MATCH_MANY_MAX_QUERIES, MATCH_MANY_MAX_OPS, MATCH_MANY_MAX_CONDS

    def __init__(self, expressions):
        expressions = list(expressions)
        if len(expressions) > self.MAX_QUERIES:
            raise ValueError(f"{len(expressions)} queries: one batched match call holds {self.MAX_QUERIES}")
        self.kinds: list[int] = []
        self.fields: list[bytes] = []
        self.tokens: list[bytes] = []
        self.prog_ops: list[int] = []
        self.prog_off: list[int] = [0]
        self.index_maps: list[list[int]] = []          # per query: CompiledMatcher condition index -> table index
        index: dict = {}
        lowered = 0
        for e in expressions:
            m = self._compile(e)
            remap = []
            for key in zip(m.kinds, m.fields, m.tokens):
                i = index.get(key)
                if i is None:
                    i = index[key] = len(self.kinds)
                    self.kinds.append(key[0])
                    self.fields.append(key[1])
                    self.tokens.append(key[2])
                remap.append(i)
            if len(self.kinds) > self.MAX_CONDS:
                raise ValueError(f"more than {self.MAX_CONDS} distinct conditions in one batched match call")
            if self.kinds.count(KIND_FIELD_REGEX) > MATCH_MANY_MAX_REGEX_CONDS:
                raise ValueError(f"more than {MATCH_MANY_MAX_REGEX_CONDS} distinct regex conditions in one batched match call")
            self.index_maps.append(remap)
            self.prog_ops.extend(op(OP_TERM, remap[o & 0x0FFFFFFF]) if (o >> 28) == OP_TERM else o for o in m.prog_ops)
            self.prog_off.append(len(self.prog_ops))
            lowered += lowered_ops(m.prog_ops)
            if lowered > self.MAX_OPS:
                raise ValueError(f"the batch's programs lower to more than {self.MAX_OPS} ops")

    @staticmethod
    def _compile(expression):
        return CompiledMatcher(expression)

    @property
    def n_queries(self) -> int:
        return len(self.prog_off) - 1


class CompiledRowQuery(CompiledMatcher):
    """The whole compileRowMatcher root And(bloom root, regex root) (row_matcher.go:353-368) for bsg_match_rows_regex: the
    bloom side lowered as CompiledMatcher does, the regex side by compileRegexExpression's rules (row_matcher.go:440-480) —
    a nil expression or condition is TRUE, an empty field FALSE, an empty Or FALSE, an empty And TRUE.  A FieldRegex
    condition keeps its field in `fields` and its pattern in `tokens` (entry 2i + 1)."""

    def __init__(self, bloom_expression, regex_expression):
        super().__init__(None)
        if bloom_expression is None:
            self.prog_ops.append(op(OP_TRUE))
        else:
            self._emit(bloom_expression)
        self._emit_regex(regex_expression)
        self.prog_ops.append(op(OP_AND, 2))

    def _emit_regex(self, e) -> None:
        if e is None:
            self.prog_ops.append(op(OP_TRUE))
            return
        et = e.get("ExpressionType")
        if et == EXPR_CONDITION:
            cond = e.get("Condition")
            if cond is None:
                self.prog_ops.append(op(OP_TRUE))
            elif cond.get("Field", "") == "":
                self.prog_ops.append(op(OP_FALSE))
            else:
                self.prog_ops.append(op(OP_TERM, len(self.kinds)))
                self.kinds.append(KIND_FIELD_REGEX)
                self.fields.append(cond["Field"].encode("utf-8", "surrogatepass"))
                self.tokens.append(cond.get("Pattern", "").encode("utf-8", "surrogatepass"))
        elif et in (EXPR_AND, EXPR_OR):
            kids = e.get("Children") or []
            if not kids:
                self.prog_ops.append(op(OP_TRUE if et == EXPR_AND else OP_FALSE))
                return
            for c in kids:
                self._emit_regex(c)
            self.prog_ops.append(op(OP_AND if et == EXPR_AND else OP_OR, len(kids)))
        else:
            self.prog_ops.append(op(OP_FALSE))


class CompiledSubstringQuery(CompiledMatcher):
    """And(bloom root, substring root) for bsg_match_rows_substr: the bloom side lowered as CompiledMatcher does, the substring
    side by the regex tree's rules (a nil expression or condition is TRUE, an empty Or FALSE, an empty And TRUE).  A Substring
    condition keeps an empty field, a FieldSubstring condition its field, both the RAW needle in `tokens` (entry 2i + 1)."""

    def __init__(self, bloom_expression, substring_expression):
        super().__init__(None)
        if bloom_expression is None:
            self.prog_ops.append(op(OP_TRUE))
        else:
            self._emit(bloom_expression)
        self._emit_substring(substring_expression)
        self.prog_ops.append(op(OP_AND, 2))

    def _emit_substring(self, e) -> None:
        if e is None:
            self.prog_ops.append(op(OP_TRUE))
            return
        et = e.get("ExpressionType")
        if et == EXPR_CONDITION:
            cond = e.get("Condition")
            if cond is None:
                self.prog_ops.append(op(OP_TRUE))
                return
            field = cond.get("Field")
            self.prog_ops.append(op(OP_TERM, len(self.kinds)))
            self.kinds.append(KIND_SUBSTRING if field is None else KIND_FIELD_SUBSTRING)
            self.fields.append(b"" if field is None else field.encode("utf-8", "surrogatepass"))
            needle = cond.get("Needle", "")
            self.tokens.append(needle if isinstance(needle, bytes) else needle.encode("utf-8", "surrogatepass"))
        elif et in (EXPR_AND, EXPR_OR):
            kids = e.get("Children") or []
            if not kids:
                self.prog_ops.append(op(OP_TRUE if et == EXPR_AND else OP_FALSE))
                return
            for c in kids:
                self._emit_substring(c)
            self.prog_ops.append(op(OP_AND if et == EXPR_AND else OP_OR, len(kids)))
        else:
            self.prog_ops.append(op(OP_FALSE))


class CompiledRangeQuery(CompiledMatcher):
    """And(bloom root | TRUE, range root) for bsg_match_rows_range: the bloom side lowered as CompiledMatcher does, the range side by
    the regex tree's rules (a nil expression or condition is TRUE, an empty field FALSE, an empty Or FALSE, an empty And TRUE).  A
    FieldRange condition keeps its field in `fields` and range_entry's 17 bytes in `tokens` (entry 2i + 1)."""

    def __init__(self, bloom_expression, range_expression):
        super().__init__(None)
        if bloom_expression is None:
            self.prog_ops.append(op(OP_TRUE))
        else:
            self._emit(bloom_expression)
        self._emit_range(range_expression)
        self.prog_ops.append(op(OP_AND, 2))

    def _emit_range(self, e) -> None:
        if e is None:
            self.prog_ops.append(op(OP_TRUE))
            return
        et = e.get("ExpressionType")
        if et == EXPR_CONDITION:
            cond = e.get("Condition")
            if cond is None:
                self.prog_ops.append(op(OP_TRUE))
            elif cond.get("Field", "") == "":
                self.prog_ops.append(op(OP_FALSE))
            else:
                self.prog_ops.append(op(OP_TERM, len(self.kinds)))
                self.kinds.append(KIND_FIELD_RANGE)
                self.fields.append(cond["Field"].encode("utf-8", "surrogatepass"))
                self.tokens.append(range_entry(cond))
        elif et in (EXPR_AND, EXPR_OR):
            kids = e.get("Children") or []
            if not kids:
                self.prog_ops.append(op(OP_TRUE if et == EXPR_AND else OP_FALSE))
                return
            for c in kids:
                self._emit_range(c)
            self.prog_ops.append(op(OP_AND if et == EXPR_AND else OP_OR, len(kids)))
        else:
            self.prog_ops.append(op(OP_FALSE))


class CompiledRangeQueryBatch(CompiledMatcherBatch):
    """A batch of (bloom expression, range expression) pairs for one bsg_match_rows_many_range call: query q's program is
    CompiledRangeQuery's with its condition indices remapped into ONE table of distinct conditions (a range condition is distinct by
    its field, bounds and flags)."""

    @staticmethod
    def _compile(pair):
        return CompiledRangeQuery(*pair)


class CompiledSubstringQueryBatch(CompiledMatcherBatch):
    """A batch of (bloom expression, substring expression) pairs for one bsg_match_rows_many_substr call: query q's program is
    CompiledSubstringQuery's with its condition indices remapped into ONE table of distinct conditions."""

    @staticmethod
    def _compile(pair):
        return CompiledSubstringQuery(*pair)


class CompiledRowSubstringQuery(CompiledRowQuery, CompiledSubstringQuery):
    """And(bloom root | TRUE, regex root, substring root) for bsg_match_rows_regex_substr: the bloom side lowered as CompiledMatcher does,
    the regex side by CompiledRowQuery's rules (an empty field is FALSE), the substring side by CompiledSubstringQuery's; FieldRegex,
    Substring and FieldSubstring conditions share the one table."""

    def __init__(self, bloom_expression, regex_expression, substring_expression):
        CompiledMatcher.__init__(self, None)
        if bloom_expression is None:
            self.prog_ops.append(op(OP_TRUE))
        else:
            self._emit(bloom_expression)
        self._emit_regex(regex_expression)
        self._emit_substring(substring_expression)
        self.prog_ops.append(op(OP_AND, 3))


class CompiledRowSubstringQueryBatch(CompiledMatcherBatch):
    """A batch of (bloom expression, regex expression, substring expression) triples for one bsg_match_rows_many_regex_substr call: query
    q's program is CompiledRowSubstringQuery's with its condition indices remapped into ONE table of distinct conditions, deduplicated
    by (kind, field, token / pattern / needle).  Raises ValueError beyond 64 queries, 64 conditions, 2 048 lowered ops or 16 regex
    conditions."""

    @staticmethod
    def _compile(triple):
        return CompiledRowSubstringQuery(*triple)


class CompiledRowTextRangeQuery(CompiledRowQuery, CompiledSubstringQuery, CompiledRangeQuery):
    """And(bloom root | TRUE, regex root, substring root, range root) for bsg_match_rows_regex_substr_range: each side lowered by its own
    parent's rules (CompiledMatcher, CompiledRowQuery, CompiledSubstringQuery, CompiledRangeQuery); FieldRegex, Substring,
    FieldSubstring and FieldRange conditions share the one table."""

    def __init__(self, bloom_expression, regex_expression, substring_expression, range_expression):
        CompiledMatcher.__init__(self, None)
        if bloom_expression is None:
            self.prog_ops.append(op(OP_TRUE))
        else:
            self._emit(bloom_expression)
        self._emit_regex(regex_expression)
        self._emit_substring(substring_expression)
        self._emit_range(range_expression)
        self.prog_ops.append(op(OP_AND, 4))


class CompiledRowTextRangeQueryBatch(CompiledMatcherBatch):
    """A batch of (bloom, regex, substring, range) expression quadruples for one bsg_match_rows_many_regex_substr_range call: query q's
    program is CompiledRowTextRangeQuery's with its condition indices remapped into ONE table of distinct conditions, deduplicated by
    (kind, field, token / pattern / needle / range entry).  Raises ValueError beyond 64 queries, 64 conditions, 2 048 lowered ops or 16
    regex conditions."""

    @staticmethod
    def _compile(quad):
        return CompiledRowTextRangeQuery(*quad)


class CompiledRowQueryBatch(CompiledMatcherBatch):
    """A batch of (bloom expression, regex expression) pairs for one bsg_match_rows_many_regex call: query q's program is
    CompiledRowQuery(bloom_q, regex_q)'s with its condition indices remapped into ONE table of distinct conditions,
    deduplicated by (kind, field, token or pattern) as CompiledMatcherBatch does.  Raises ValueError beyond 64 queries, 64
    conditions, 2 048 lowered ops or 16 regex conditions."""

    @staticmethod
    def _compile(pair):
        return CompiledRowQuery(*pair)


MATCH_WIDE_MAX_QUERIES, MATCH_WIDE_MAX_OPS, MATCH_WIDE_MAX_PAIRS = 1 << 20, 1 << 22, 1 << 24      # bloomgpu.h bsg_match_rows_wide


class CompiledWideBatch(CompiledRowQueryBatch):
    """Any number of queries for one bsg_match_rows_wide call: the table and the programs exactly as CompiledRowQueryBatch builds
    them — ONE table of at most 64 distinct conditions (16 of them regex), query q's program CompiledRowQuery's (for a
    (bloom, regex) pair) or CompiledMatcher's (for a plain expression, or None) with its indices remapped — without the 64-query and
    2 048-op limits of the batched calls.  Raises ValueError beyond 2^20 queries, 2^22 lowered ops, 64 conditions, 16 regex conditions."""

    MAX_QUERIES, MAX_OPS = MATCH_WIDE_MAX_QUERIES, MATCH_WIDE_MAX_OPS

    @staticmethod
    def _compile(item):
        return CompiledRowQuery(*item) if isinstance(item, tuple) else CompiledMatcher(item)


class CompiledWideSubstringBatch(CompiledRowSubstringQueryBatch):
    """Any number of (bloom expression, regex expression, substring expression) triples for one bsg_match_rows_wide_substr call: the
    table and the programs exactly as CompiledRowSubstringQueryBatch builds them, without the 64-query and 2 048-op limits of the
    batched calls.  Raises ValueError beyond 2^20 queries, 2^22 lowered ops, 64 conditions or 16 regex conditions."""

    MAX_QUERIES, MAX_OPS = MATCH_WIDE_MAX_QUERIES, MATCH_WIDE_MAX_OPS


class CompiledWideRangeBatch(CompiledRangeQueryBatch):
    """Any number of (bloom expression, range expression) pairs for one bsg_match_rows_wide_range call: the table and the programs
    exactly as CompiledRangeQueryBatch builds them, without the 64-query and 2 048-op limits of the batched call.  Raises ValueError
    beyond 2^20 queries, 2^22 lowered ops or 64 distinct conditions."""

    MAX_QUERIES, MAX_OPS = MATCH_WIDE_MAX_QUERIES, MATCH_WIDE_MAX_OPS


class CompiledWideTextRangeBatch(CompiledRowTextRangeQueryBatch):
    """Any number of (bloom, regex, substring, range) expression quadruples for one bsg_match_rows_wide_regex_substr_range call: the table
    and the programs exactly as CompiledRowTextRangeQueryBatch builds them, without the 64-query and 2 048-op limits of the batched
    call.  Raises ValueError beyond 2^20 queries, 2^22 lowered ops, 64 conditions or 16 regex conditions."""

    MAX_QUERIES, MAX_OPS = MATCH_WIDE_MAX_QUERIES, MATCH_WIDE_MAX_OPS

    def __init__(self, quadruples):
        quadruples = list(quadruples)
        super().__init__(quadruples)
        self.queries = quadruples                  # what histogram() decides the handed-back rows with

    def histogram(self, ctx, rows, field, origin: int, width: int, n_buckets: int, set_first_row=None, set_query_off=None, set_queries=None,
                  tokenizer=None):
        """Per (set, query) pair, how many matching rows fall into each bucket of the top-level number field: ctx.match_rows_wide_hist
        (bsg_match_rows_wide_hist), then every row the device handed back decided on the host — its match by the four host matchers,
        its slot by bsh_hist_row — and added.  -> u32 counts [n_pairs, n_buckets + 3] (the buckets, then below, above, missing): final."""
        from . import host
        counts, handed_back = ctx.match_rows_wide_hist(rows, self, field, origin, width, n_buckets, set_first_row, set_query_off, set_queries, tokenizer)
        counts = counts.copy()
        if len(handed_back) == 0:
            return counts
        if isinstance(rows, tuple):
            blob, off = bytes(np.asarray(rows[0], dtype=np.uint8)), np.asarray(rows[1], dtype=np.uint64)
            row_of = lambda r: blob[int(off[r]): int(off[r + 1])]
        else:
            row_of = lambda r: rows[r]
        if set_first_row is None:
            first, pair_off, pairs = np.array([0, 1 << 32], dtype=np.uint64), [0, self.n_queries], list(range(self.n_queries))
        else:
            first, pair_off, pairs = np.asarray(set_first_row, dtype=np.uint64), [int(x) for x in set_query_off], [int(q) for q in set_queries]
        for r in handed_back:
            row = row_of(int(r))
            s = int(np.searchsorted(first, int(r), side="right")) - 1
            slot = None
            for p in range(pair_off[s], pair_off[s + 1]):
                bloom, regex, sub, rng = self.queries[pairs[p]]
                if (bloom is None or host.match_row(bloom, row, tokenizer)) and host.match_row_regex(regex, row) and \
                        host.match_row_substring(sub, row, tokenizer) and host.match_row_range(rng, row):
                    if slot is None:
                        slot = host.hist_row(row, field, origin, width, n_buckets)
                    counts[p, slot] += 1
        return counts


MATCH_LOOKUP_MAX_CONDS = 1024                                                   # bloomgpu.h BSG_MATCH_LOOKUP_MAX_CONDS


class CompiledLookupBatch(CompiledWideBatch):
    """Any number of queries for one bsg_match_rows_lookup call: CompiledWideBatch's table and programs over at most 1 024 distinct
    Field / Token / FieldToken conditions.  Raises ValueError beyond 2^20 queries, 2^22 lowered ops or 1 024 distinct conditions, and
    on a FieldRegex condition (batches with one take CompiledLookupRegexBatch or CompiledWideBatch)."""

    MAX_CONDS = MATCH_LOOKUP_MAX_CONDS

    @staticmethod
    def _compile(item):
        m = CompiledWideBatch._compile(item)
        if KIND_FIELD_REGEX in m.kinds:
            raise ValueError("a FieldRegex condition: the lookup match call holds Field, Token and FieldToken conditions only")
        return m


class CompiledLookupRegexBatch(CompiledWideBatch):
    """Any number of queries for one bsg_match_rows_lookup_regex call: CompiledWideBatch's items ((bloom, regex) pairs included), table
    and programs over at most 1 024 distinct conditions, at most 16 of them FieldRegex.  Raises ValueError beyond 2^20 queries, 2^22
    lowered ops, 1 024 distinct conditions or 16 distinct regex conditions (the message says which)."""

    MAX_CONDS = MATCH_LOOKUP_MAX_CONDS
