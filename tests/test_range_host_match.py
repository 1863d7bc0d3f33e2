"""host/range.hpp through bsh_match_row_range / bsh_prune_query_range: the exact range test of a row against a plain-Python restatement
(tests/range_restatement.py: Fractions of the raw literals), for every literal x every pair of bounds, the path and leaf rules, the
lowering of the reference's ten numeric operators, and the range guard as the fourth side of the pruning expression."""
import fractions

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import range_restatement as RR


@pytest.mark.parametrize("literal", RR.LITERALS)
def test_every_literal_against_every_pair_of_bounds(literal):
    row = ('{"v":%s}' % literal).encode()
    value = RR.exact(literal)
    assert list(RR.number_leaves(RR.parse(row))) == [("v", value)]
    for lo, hi in RR.BOUND_PAIRS:
        got = Hst.match_row_range(RR.field_range(Q, "v", lo, hi), row)
        assert got == RR.inside(value, lo, hi), (literal, lo, hi)


def test_the_pinned_values():
    def m(lit, lo=None, hi=None, **kw):
        return Hst.match_row_range(Q.FieldRange("v", lo, hi, **kw), ('{"v":%s}' % lit).encode())
    assert m("9007199254740993", 9007199254740993, 9007199254740993) and not m("9007199254740993", 9007199254740992, 9007199254740992)
    assert m("5.000", 5, 5) and not m("5.0001", 5, 5) and m("5.0001", 5, None, lo_open=True)
    assert m("-0", 0, 0) and m("-0.0", 0, 0) and not m("-0.0", None, 0, hi_open=True)
    assert m("-5.5", -6, -5) and not m("-5.5", -5, None) and m("-5.5", None, -5, hi_open=True)
    assert not m("9223372036854775808", None, RR.I64_MAX) and m("9223372036854775808", RR.I64_MAX, None, lo_open=True)
    assert not m("-9223372036854775809", RR.I64_MIN, None) and m("-9223372036854775808", RR.I64_MIN, RR.I64_MIN)
    assert m(RR.BIG, 0, None) and not m(RR.BIG, None, RR.I64_MAX) and m("-" + RR.BIG, None, RR.I64_MIN, hi_open=True)
    assert m("1e3", 1000, 1000) and m("123456789e-3", 123456, 123457) and not m("123456789e-3", 123457, None)
    assert m("-1e-400", -1, 0) and not m("-1e-400", 0, None) and m("1E+21", RR.I64_MAX, None) and m("1e400", 0, None) and m("2.5e-7", 0, 1, lo_open=True)
    assert not m("7", 9, 3)                                                     # lo > hi is valid and never holds
    assert not m('"5"', 5, 5) and not m("true") and not m("null") and m("5")    # no bounds: any number, and only a number


def test_path_and_leaf_rules():
    for row, checks in RR.PATH_CASES:
        for field, (lo, hi), expected in checks:
            tree = RR.field_range(Q, field, lo, hi)
            assert RR.row_verdict(row, tree) == expected, (row, field, lo, hi)
            assert Hst.match_row_range(tree, row) == expected, (row, field, lo, hi)


def test_trees_and_the_nil_rules():
    row = b'{"a":5,"b":[1,2.5],"c":"x"}'
    A, B = Q.FieldRange("a", 5, 5), Q.FieldRange("b", 2, 3, lo_open=True)
    trees = [None, A, B, Q.RangeAnd(A, B), Q.RangeOr(Q.FieldRange("a", 6, None), B), Q.RangeAnd(A, Q.FieldRange("c", None, None)), Q.RangeAnd(), Q.RangeOr(),
             Q.RangeOr(Q.NIL_CONDITION, Q.FieldRange("a", 6, None)), Q.RangeAnd(Q.NIL_CONDITION, Q.FieldRange("a", 6, None)), {"ExpressionType": "NOT"},
             Q.FieldRange("", None, None)]
    want = [True, True, True, True, True, False, True, False, True, False, False, False]
    assert [RR.row_verdict(row, t) for t in trees] == want
    assert [Hst.match_row_range(t, row) for t in trees] == want
    assert Hst.match_row_range(A, b'{"a":5') is False                           # a row that is not valid JSON
    with pytest.raises(Hst.HostError):
        Hst.match_row_range({"ExpressionType": "CONDITION", "Condition": {"Field": "a", "Lo": 1.5}}, row)
    with pytest.raises(Hst.HostError):
        Hst.match_row_range({"ExpressionType": "CONDITION", "Condition": {"Field": "a", "Hi": 1 << 63}}, row)
    with pytest.raises(ValueError):
        Q.FieldRange("a", 1 << 63)


OPERATORS = {
    "EQ": lambda x, c: x == c["Value"], "NE": lambda x, c: x != c["Value"], "GT": lambda x, c: x > c["Value"], "GTE": lambda x, c: x >= c["Value"],
    "LT": lambda x, c: x < c["Value"], "LTE": lambda x, c: x <= c["Value"], "IN": lambda x, c: x in c["Values"], "NOT_IN": lambda x, c: x not in c["Values"],
    "BETWEEN": lambda x, c: c["Min"] <= x <= c["Max"], "NOT_BETWEEN": lambda x, c: not (c["Min"] <= x <= c["Max"]),
}


def test_the_ten_numeric_operators_lower_to_range_trees():
    conds = [{"Operator": o, "Value": v} for o in ("EQ", "NE", "GT", "GTE", "LT", "LTE") for v in (-5, 0, 5, RR.I64_MIN, RR.I64_MAX)]
    conds += [{"Operator": o, "Values": vs} for o in ("IN", "NOT_IN") for vs in ([], [5], [6, 5, -5], [0, 5, 5, RR.I64_MAX], [RR.I64_MIN, -6, -5])]
    conds += [{"Operator": o, "Min": a, "Max": b} for o in ("BETWEEN", "NOT_BETWEEN") for a, b in ((-5, 5), (5, 5), (6, 5), (RR.I64_MIN, 0), (0, RR.I64_MAX))]
    assert {c["Operator"] for c in conds} == set(OPERATORS)
    for c in conds:
        tree = Q.numeric_condition_range("v", c)
        for literal in RR.LITERALS:
            x = RR.exact(literal)
            row = ('{"v":%s}' % literal).encode()
            want = OPERATORS[c["Operator"]](x, c)
            assert RR.row_verdict(row, tree) == want, (c, literal)
            assert Hst.match_row_range(tree, row) == want, (c, literal)
    with pytest.raises(ValueError):
        Q.numeric_condition_range("v", {"Operator": "LIKE"})
    # "some leaf": NE holds for an array that has another value
    assert Hst.match_row_range(Q.numeric_condition_range("v", {"Operator": "NE", "Value": 1}), b'{"v":[1,2]}')
    assert not Hst.match_row_range(Q.numeric_condition_range("v", {"Operator": "NE", "Value": 1}), b'{"v":[1,1.0]}')


def test_the_range_guard_is_the_fourth_side_of_the_pruning_expression():
    bloom, regex, sub = Q.FieldToken("lvl", "error"), Q.FieldRegex("msg", "^a"), Q.FieldSubstring("msg", "timeout")
    for b, r, s in [(None, None, None), (bloom, None, None), (bloom, regex, None), (bloom, regex, sub), (None, None, sub)]:
        assert Hst.prune_query_range(b, r, s, None) == Hst.prune_query_sub(b, r, s)           # a nil range tree
    rng = Q.FieldRange("ts", 10, 20)
    assert Hst.prune_query_range(None, None, None, rng) == Q.Field("ts")
    assert Hst.prune_query_range(bloom, None, None, rng) == Q.And(bloom, Q.Field("ts"))
    three = Hst.prune_query_sub(bloom, regex, sub)
    assert Hst.prune_query_range(bloom, regex, sub, rng) == Q.and_bloom_queries(three, Q.Field("ts"))
    # the bounds play no part; And and Or keep their shape
    tree = Q.RangeAnd(Q.FieldRange("a", 1, None), Q.RangeOr(Q.FieldRange("b", None, 2), Q.FieldRange("c", 3, 3)))
    assert Hst.prune_query_range(None, None, None, tree) == Q.range_guard_bloom_query(tree) == \
        {"ExpressionType": "AND", "Children": [Q.Field("a"), {"ExpressionType": "OR", "Children": [Q.Field("b"), Q.Field("c")]}]}
    # the nil condition is always true: an Or keeps it (and stays true), an And drops it
    with_nil = Q.RangeOr(Q.NIL_CONDITION, Q.FieldRange("a", 1, 2))
    assert Hst.prune_query_range(None, None, None, with_nil) == Q.range_guard_bloom_query(with_nil) == \
        {"ExpressionType": "OR", "Children": [Q.NIL_CONDITION, Q.Field("a")]}
    and_nil = Q.RangeAnd(Q.NIL_CONDITION, Q.FieldRange("a", 1, 2))
    assert Hst.prune_query_range(None, None, None, and_nil) == Q.range_guard_bloom_query(and_nil) == {"ExpressionType": "AND", "Children": [Q.Field("a")]}
    assert Hst.prune_query_range(None, None, None, Q.RangeAnd(Q.NIL_CONDITION)) is None
    assert Hst.prune_query_range(bloom, None, None, Q.RangeAnd(Q.NIL_CONDITION)) == bloom


def test_the_compiled_query_packs_bounds_and_flags():
    m = Q.CompiledRangeQuery(Q.Field("x"), Q.RangeOr(Q.FieldRange("a", -2, None, lo_open=True), Q.FieldRange("", 1, 2), Q.FieldRange("b", None, RR.I64_MAX)))
    assert m.kinds == [0, 6, 6] and m.fields == [b"x", b"a", b"b"]
    assert m.tokens[1] == (-2).to_bytes(8, "little", signed=True) + bytes(8) + bytes([2 | 4])
    assert m.tokens[2] == bytes(8) + RR.I64_MAX.to_bytes(8, "little", signed=True) + bytes([1])
    assert all(len(t) == 17 for t in m.tokens[1:])
    batch = Q.CompiledRangeQueryBatch([(None, Q.FieldRange("a", 1, 2)), (Q.Field("x"), Q.FieldRange("a", 1, 2)), (None, Q.FieldRange("a", 1, 2, hi_open=True))])
    assert batch.kinds == [6, 0, 6] and batch.n_queries == 3
    assert fractions.Fraction(1, 2) == RR.exact("0.5")
