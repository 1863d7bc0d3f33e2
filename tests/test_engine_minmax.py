"""MinMaxIndexes and Prefilter on the host side of the engine mirror, without a device: the config key is checked with the C ABI's
limits before the context is looked at, and the query builders emit the reference's JSON shape, which the host's prefilter tree reads
back to the restatement's verdicts."""
import ctypes as C
import json

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import minmax_restatement as MR


def open_rc(**config):
    L = Hst.lib()
    cfg = json.dumps(config).encode()
    h = C.c_void_p()
    rc = L.bse_open(cfg, len(cfg), None, C.byref(h))
    assert not h.value
    return rc


@pytest.mark.parametrize("bad", [["ts", "ts"], [""], ["x" * 65], ["f%d" % i for i in range(9)], "ts", [1], {"ts": 1}],
                         ids=["equal", "empty", "65 bytes", "nine", "a string", "a number", "an object"])
def test_an_invalid_list_is_an_invalid_config(bad):
    assert open_rc(MinMaxIndexes=bad) == -101                      # BSE_E_INVALID_CONFIG, before the NULL context is looked at


@pytest.mark.parametrize("good", [["ts"], ["f%d" % i for i in range(8)], ["x" * 64, "a.b"], [], None], ids=["one", "eight", "64 bytes", "empty", "null"])
def test_a_valid_list_passes_the_config_check(good):
    assert open_rc(MinMaxIndexes=good) == -1                       # BSH_E_INVALID: the config was fine, the context is NULL
    assert open_rc(MinMaxIndexes=good, DeviceIngest=True, DeviceIngestStream=True) == -1


def test_the_builders_emit_the_reference_shape():
    assert Q.MinMax("ts", "GTE", 5) == {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "MINMAX", "MinMaxFieldName": "ts",
                                                                                       "MinMaxCondition": {"Operator": "GTE", "Value": 5}}}
    assert Q.MinMax("ts", "BETWEEN", -1, 1)["Condition"]["MinMaxCondition"] == {"Operator": "BETWEEN", "Min": -1, "Max": 1}
    assert Q.MinMax("ts", "IN", 1, 2)["Condition"]["MinMaxCondition"] == {"Operator": "IN", "Values": [1, 2]}
    assert Q.Partition("EQ", "p") == {"ExpressionType": "CONDITION", "Condition": {"ConditionType": "PARTITION", "PartitionCondition": {"Operator": "EQ", "Value": "p"}}}
    assert Q.Partition("NOT_IN", "a", "b")["Condition"]["PartitionCondition"] == {"Operator": "NOT_IN", "Values": ["a", "b"]}
    both = Q.PrefilterAnd(Q.MinMax("ts", "LT", 3), Q.PrefilterAnd(Q.Partition("NE", "x"), Q.PrefilterOr()))
    assert both["ExpressionType"] == "AND" and [c["ExpressionType"] for c in both["Children"]] == ["CONDITION", "CONDITION", "OR"]
    for bad in (lambda: Q.MinMax("ts", "GTE", 1 << 63), lambda: Q.MinMax("ts", "GTE", 1.5), lambda: Q.MinMax("ts", "LIKE", 1), lambda: Q.Partition("EQ", 5),
                lambda: Q.MinMax("ts", "BETWEEN", 1), lambda: Q.MinMax("ts", "EQ", True)):
        with pytest.raises(ValueError):
            bad()


def test_the_host_tree_reads_the_builders_output():
    blocks = [("p1", {"ts": (100, 199)}), ("p2", {"ts": (200, 299), "u": (-5, 5)}), ("", {"ts": (0, 99)}), ("p3", {})]
    trees = [Q.MinMax("ts", op, 150) for op in ("EQ", "NE", "GT", "GTE", "LT", "LTE")] + [
        Q.MinMax("ts", "IN", 99, 300), Q.MinMax("ts", "NOT_IN", 99), Q.MinMax("ts", "BETWEEN", 199, 200), Q.MinMax("ts", "NOT_BETWEEN", 100, 199),
        Q.MinMax("u", "LTE", -5), Q.Partition("GT", "p1"), Q.Partition("NOT_BETWEEN", "p2", "p3"),
        Q.PrefilterOr(Q.MinMax("ts", "LT", 100), Q.Partition("EQ", "p3")), Q.PrefilterAnd(Q.MinMax("ts", "GTE", 100), Q.Partition("IN", "p2", "p3"))]
    for t in trees:
        for pid, idx in blocks:
            assert Hst.prefilter_eval(t, pid, idx) == MR.prefilter_holds(t, pid, idx), (t, pid)
