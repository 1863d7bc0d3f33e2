"""The MinMax index on the host: the shapes' stated contributions against the restatement, bsh_minmax_row (host/minmax.hpp) against
the restatement for every literal, every shape and the giants, bsh_minmax_eval against the restatement's evaluate over the int64 edges
and saturated indexes, and the prefilter tree's empty-Or, empty-And, nil and missing-index rules."""
import itertools

import numpy as np
import pytest

from bloomsearch_amd import _lib, host
from tests import minmax_restatement as MR
from tests import minmax_shapes as MS

I64_MIN, I64_MAX = MR.I64_MIN, MR.I64_MAX


def host_row(row, fields):
    """{field: (min, max)} bsh_minmax_row folds into an absent index"""
    rec = host.minmax_row(row, fields)
    return {f: (int(rec["min"][i]), int(rec["max"][i])) for i, f in enumerate(fields) if rec["present"][i]}


@pytest.mark.parametrize("shape", MS.SHAPES, ids=lambda s: s.name)
def test_a_shape_contributes_what_it_names(shape):
    assert MR.row_contributions(shape.row, MS.FIELDS) == shape.want
    assert host_row(shape.row, MS.FIELDS) == shape.want


def test_the_shapes_cover_the_contract():
    assert len(MS.UNDECIDED) >= 9 and all(b"e" in s.row.lower() or b"\\" in s.row for s in MS.UNDECIDED)
    assert any(len(s.row) > 300 for s in MS.SHAPES)
    want = {name: MR.set_indexes(row_sets, fields) for name, row_sets, fields in MS.batches()}
    assert want["an empty set between two others"][1] == [None] * 3
    assert want["a set without the key"][1] == [None] * 3
    assert want["a set where every row is handed back"][1][0] is not None        # the folded result of that set is not absent
    eight = want["eight fields, hits on the first and the eighth"]
    assert eight[0] == [(-40, 89)] + [None] * 6 + [(871, 1000)] and eight[1] == [None] * 7 + [(-8, -7)]
    assert [len(rs[0]) for _, rs, _ in MS.batches()[:5]] == [1, 63, 64, 65, 513]


@pytest.mark.parametrize("literal", MR.LITERALS + [MR.BIG + "." + MR.BIG, "-0." + "0" * 40 + "1", "0." + "9" * 40, "-" + MR.BIG + "e-39", "1e19", "1e18",
                                                   "9.223372036854775807e18", "9.223372036854775808e18", "-9.223372036854775808e18", "-9.2233720368547758081e18",
                                                   "0.0000001e7", "123.456e2", "123.456e1", "1e-0", "-1E-1"])
def test_the_host_decides_every_literal(literal):
    row = ('{"v":%s,"w":"x"}' % literal).encode()
    assert host_row(row, ["v"]) == {"v": MR.contribution_of(MR.exact(literal))}


def test_the_giants():
    """exponents no Fraction should be asked to hold: the results are stated"""
    for lit, want in [("1e99999999999999999999", (I64_MAX, I64_MAX)), ("-1e99999999999999999999", (I64_MIN, I64_MIN)),
                      ("1e-99999999999999999999", (0, 1)), ("-1e-99999999999999999999", (-1, 0)), ("0e99999999999999999999", (0, 0)),
                      ("-0.000e-99999999999999999999", (0, 0))]:
        assert host_row(('{"v":%s}' % lit).encode(), ["v"]) == {"v": want}, lit


def test_the_fold_and_the_rows_that_are_no_objects():
    rec = np.zeros(2, dtype=_lib.MINMAX_DTYPE)
    for row in [b'{"a":5,"b":-1}', b'{"a":-7.5}', b'{"a":"x","b":3}', b'{"c":1}']:
        host.minmax_row(row, ["a", "b"], rec)
    assert [tuple(int(x) for x in r) for r in rec[["min", "max", "present"]].tolist()] == [(-8, 5, 1), (-1, 3, 1)]
    before = rec.copy()
    for row in MS.MALFORMED:
        with pytest.raises(host.HostError):
            host.minmax_row(row, ["ts", "m"], rec)
    assert np.array_equal(before, rec)
    for bad in ([], ["x"] * 2, [""], ["y" * 65], ["f%d" % i for i in range(9)]):
        with pytest.raises(host.HostError):
            host.minmax_row(b'{"x":1}', bad)
    assert host_row(b'{"%s":1}' % (b"y" * 64), ["y" * 64]) == {"y" * 64: (1, 1)}


EDGES = [I64_MIN, I64_MIN + 1, -6, -5, 0, 5, 6, I64_MAX - 1, I64_MAX]
INDEXES = [(a, b) for a, b in itertools.combinations_with_replacement(EDGES, 2)]


@pytest.mark.parametrize("op", MR.OPS)
def test_eval_against_the_restatement(op):
    bad = []
    for idx in INDEXES:
        if op in ("BETWEEN", "NOT_BETWEEN"):
            args = [dict(lo=lo, hi=hi) for lo, hi in itertools.product(EDGES, EDGES)]
        elif op in ("IN", "NOT_IN"):
            args = [dict(values=vs) for vs in ([], [0], [I64_MIN], [I64_MAX], [-6, 6], [I64_MIN + 1, I64_MAX - 1, 5])]
        else:
            args = [dict(value=v) for v in EDGES]
        for a in args:
            if host.minmax_eval(idx[0], idx[1], op, **a) != MR.evaluate(idx, op, **a):
                bad.append((idx, a))
    assert not bad, bad[:5]


def test_eval_saturation_is_stated():
    assert host.minmax_eval(I64_MAX, I64_MAX, "GT", I64_MAX) and host.minmax_eval(I64_MAX, I64_MAX, "NE", I64_MAX)
    assert host.minmax_eval(I64_MIN, I64_MIN, "LT", I64_MIN) and host.minmax_eval(I64_MIN, I64_MIN, "NOT_BETWEEN", lo=I64_MIN, hi=I64_MAX)
    assert not host.minmax_eval(5, 5, "NE", 5) and not host.minmax_eval(5, 6, "GT", 6) and not host.minmax_eval(5, 6, "LT", 5)
    assert host.minmax_eval(5, 6, "NOT_IN", values=[5, 6]) and not host.minmax_eval(5, 6, "IN", values=[4, 7])
    with pytest.raises(host.HostError):
        host.minmax_eval(0, 0, 10)


def cond_mm(field, op, **kw):
    return {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "MINMAX", "MinMaxFieldName": field,
                                                           "MinMaxCondition": None if op is None else dict({"Operator": op}, **kw)}}


def cond_part(op, **kw):
    return {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "PARTITION", "PartitionCondition": None if op is None else dict({"Operator": op}, **kw)}}


def tree(t, *kids):
    return {"ExpressionType": t, "Children": list(kids)}


TREES = [
    None, tree("OR"), tree("AND"), {"ExpressionType": "CONDITION", "Condition": None}, {"ExpressionType": "NOPE"},
    cond_mm("ts", "GTE", Value=100), cond_mm("ts", "LT", Value=100), cond_mm("missing", "GTE", Value=I64_MIN), cond_mm("missing", "NOT_IN", Values=[1]),
    cond_mm("ts", None), cond_mm("missing", None), cond_mm("ts", "BETWEEN", Min=50, Max=60), cond_mm("ts", "IN", Values=[1, 150]),
    cond_mm("ts", "XX", Value=1), cond_part("EQ", Value="p1"), cond_part("NE", Value="p1"), cond_part(None), cond_part("IN", Values=["p0", "p2"]),
    cond_part("NOT_IN", Values=["p1"]), cond_part("BETWEEN", Min="p0", Max="p1"), cond_part("GT", Value="p"), cond_part("LTE", Value="p1"),
    tree("OR", cond_mm("ts", "GT", Value=1000), cond_part("EQ", Value="p1")), tree("AND", cond_mm("ts", "GT", Value=1000), cond_part("EQ", Value="p1")),
    tree("AND", tree("OR"), cond_part("EQ", Value="p1")), tree("OR", tree("AND"), cond_mm("missing", "EQ", Value=1)),
    tree("AND", cond_mm("ts", "GTE", Value=100), tree("OR", cond_part("EQ", Value="p2"), cond_mm("u", "LTE", Value=-1))),
    {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "OTHER"}},
]
BLOCKS = [("p1", {"ts": (100, 200)}), ("p2", {"ts": (0, 99), "u": (-5, -1)}), ("", {"ts": (100, 200)}), ("p1", {}), ("p0", {"u": (I64_MIN, I64_MAX)})]


@pytest.mark.parametrize("t", range(len(TREES)))
def test_the_prefilter_tree(t):
    for pid, idx in BLOCKS:
        assert host.prefilter_eval(TREES[t], pid, idx) == MR.prefilter_holds(TREES[t], pid, idx), (TREES[t], pid, idx)


def test_the_prefilter_rules_are_stated():
    pid, idx = BLOCKS[0]
    assert not host.prefilter_eval(tree("OR"), pid, idx) and host.prefilter_eval(tree("AND"), pid, idx)
    assert host.prefilter_eval({"ExpressionType": "CONDITION", "Condition": None}, pid, idx) and host.prefilter_eval(None, pid, idx)
    assert not host.prefilter_eval(cond_mm("missing", "NOT_IN", Values=[1]), pid, idx)          # a block without the index: strictly false
    assert not host.prefilter_eval(cond_part("NE", Value="zz"), "", idx)                        # an empty partition id fails every condition
    assert host.prefilter_eval(cond_part("NE", Value="zz"), "p1", idx)
