"""bsg_match_rows_regex_substr / bsg_match_rows_many_regex_substr at the C boundary, without a device: the header declares them with
the substring pair's parameter lists, the library exports them, query.CompiledRowSubstringQuery lowers the empty and nil nodes as its
two parents do, and the four LDS constants of the instances satisfy the sums their static_asserts state."""
import ctypes as C
import os
import re

from bloomsearch_amd import _lib, host as Hst, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID, OP_AND, OP_FALSE, OP_OR, OP_TERM, OP_TRUE, op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")


def params(name, text):
    m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_the_header_declares_both_calls_with_the_substring_pairs_parameters():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert params("bsg_match_rows_regex_substr", gpu_h) == params("bsg_match_rows_substr", gpu_h)
    assert params("bsg_match_rows_many_regex_substr", gpu_h) == params("bsg_match_rows_many_substr", gpu_h)
    host_h = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()
    assert params("bse_match_calls", host_h) == params("bse_describe", host_h)


def test_the_library_exports_them():
    L = _lib.load()
    H = Hst.lib()
    for name in ("bsg_match_rows_regex_substr", "bsg_match_rows_many_regex_substr"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert hasattr(H, "bse_match_calls") and "bse_match_calls" in Hst.HOST_EXPORTS
    n = C.c_uint32()
    # without a context both refuse like every entry point
    assert L.bsg_match_rows_regex_substr(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_many_regex_substr(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0,
                                              C.byref(n)) == BSG_E_INVALID


def test_compiled_row_substring_query_is_and_of_the_three_sides():
    m = Q.CompiledRowSubstringQuery(Q.FieldToken("lvl", "error"), Q.FieldRegex("msg", "timeout|refused"), Q.SubstringOr(Q.Substring("10.0.3."),
                                                                                                                    Q.FieldSubstring("ip", "10.")))
    assert m.kinds == [_lib.KIND_FIELD_TOKEN, _lib.KIND_FIELD_REGEX, _lib.KIND_SUBSTRING, _lib.KIND_FIELD_SUBSTRING]
    assert m.fields == [b"lvl", b"msg", b"", b"ip"] and m.tokens == [b"error", b"timeout|refused", b"10.0.3.", b"10."]
    assert m.prog_ops == [op(OP_TERM, 0), op(OP_TERM, 1), op(OP_TERM, 2), op(OP_TERM, 3), op(OP_OR, 2), op(OP_AND, 3)]


def test_nil_and_empty_nodes_lower_as_the_two_parents_lower_them():
    T, F = op(OP_TRUE), op(OP_FALSE)
    nil_cond = {"ExpressionType": "CONDITION", "Condition": None}
    cases = [None, nil_cond, Q.RegexAnd(), Q.RegexOr(), Q.FieldRegex("", "x"), {"ExpressionType": "NOPE"}]
    for rx in cases:
        for sx in [None, nil_cond, Q.SubstringAnd(), Q.SubstringOr(), {"ExpressionType": "NOPE"}]:
            m = Q.CompiledRowSubstringQuery(None, rx, sx)
            rx_ops = Q.CompiledRowQuery(None, rx).prog_ops[1:-1]            # [TRUE, regex side, AND 2]
            sx_ops = Q.CompiledSubstringQuery(None, sx).prog_ops[1:-1]      # [TRUE, substring side, AND 2]
            assert m.prog_ops == [T] + rx_ops + sx_ops + [op(OP_AND, 3)] and m.kinds == []
            assert set(rx_ops + sx_ops) <= {T, F}
    # the sides one by one: nil -> TRUE, an empty And -> TRUE, an empty Or -> FALSE, an empty regex field -> FALSE
    side = lambda rx, sx: Q.CompiledRowSubstringQuery(None, rx, sx).prog_ops[1:3]
    assert side(None, None) == [T, T] and side(Q.RegexAnd(), Q.SubstringAnd()) == [T, T] and side(Q.RegexOr(), Q.SubstringOr()) == [F, F]
    assert side(Q.FieldRegex("", "x"), nil_cond) == [F, T]
    # a bloom side is CompiledMatcher's; an empty-field FieldSubstring stays a condition (its path never equals a leaf's)
    m = Q.CompiledRowSubstringQuery(Q.Field("a"), None, Q.FieldSubstring("", "x"))
    assert m.kinds == [_lib.KIND_FIELD, _lib.KIND_FIELD_SUBSTRING] and m.prog_ops == [op(OP_TERM, 0), T, op(OP_TERM, 1), op(OP_AND, 3)]


def test_the_batch_deduplicates_by_kind_field_and_string():
    b = Q.CompiledRowSubstringQueryBatch([(None, Q.FieldRegex("msg", "abc"), None), (None, None, Q.FieldSubstring("msg", "abc")),
                                          (Q.FieldToken("msg", "abc"), Q.FieldRegex("msg", "abc"), Q.SubstringAnd(Q.Substring("abc"), Q.FieldSubstring("msg", "abc")))])
    assert b.n_queries == 3
    assert list(zip(b.kinds, b.fields, b.tokens)) == [(_lib.KIND_FIELD_REGEX, b"msg", b"abc"), (_lib.KIND_FIELD_SUBSTRING, b"msg", b"abc"),
                                                     (_lib.KIND_FIELD_TOKEN, b"msg", b"abc"), (_lib.KIND_SUBSTRING, b"", b"abc")]
    assert b.index_maps == [[0], [1], [2, 0, 3, 1]]
    assert b.prog_ops[b.prog_off[2]:] == [op(OP_TERM, 2), op(OP_TERM, 0), op(OP_TERM, 3), op(OP_TERM, 1), op(OP_AND, 2), op(OP_AND, 3)]


def constant(text, name):
    """the value of `constexpr uint32_t (or int) <name> = <expression>;` over the header's other constants (as tests/build_shapes.py reads its own)"""
    m = re.search(r"constexpr (?:uint32_t|int) %s = ([^;]+);" % name, text)
    assert m, name
    expr = re.sub(r"(\d+)u\b", r"\1", m.group(1))
    expr = expr.replace("~15", "-16").replace("/", "//")
    names = set(re.findall(r"\bk[A-Z]\w*", expr))
    return int(eval(expr, {"__builtins__": {}}, {n: constant(text, n) for n in names}))


def test_the_lds_constants_satisfy_the_stated_sums():
    text = open(os.path.join(CSRC, "ingest.hip.h")).read() + open(os.path.join(CSRC, "match.hip.h")).read()
    sub, many_sub = constant(text, "kMatchSubLdsBytes"), constant(text, "kMatchManySubLdsBytes")
    cap, many_cap = constant(text, "kRxSubLdsCap"), constant(text, "kRxManySubLdsCap")
    assert (sub, many_sub) == (37376 + 4096, 43780 + 12 + 4096) == (41472, 47888)
    assert cap == 80 * 1024 - sub == 40448 and many_cap == 80 * 1024 - many_sub == 34032
    for base, c in ((sub, cap), (many_sub, many_cap)):
        assert 2 * (base + c) <= 160 * 1024                 # two workgroups per CU
        assert c < 0x10000 and base % 16 == 0               # the blob's 16-bit offsets reach all of it; the table in front is 16-byte aligned
    assert cap < constant(text, "kRxLdsCap") == 44544 and many_cap < constant(text, "kRxManyLdsCap") == 38140
    groups = open(os.path.join(CSRC, "host", "regex_groups.hpp")).read()
    assert constant(groups, "kSingleSubLdsCap") == cap and constant(groups, "kManySubLdsCap") == many_cap
