"""The engine mirror's query_many with Substring trees: under DeviceMatch the substring queries stay in the batch's groups and a
group with needles is decided by ONE bsg_match_rows_many_substr / bsg_match_rows_many_regex_substr call — under the wide keys by ONE
bsg_match_rows_wide_substr(_rows) call — instead of one single-query call each.  Every answer is query()'s and the restatements'
(tests/test_engine_regex_substr_gpu.restated); Engine.match_calls() shows the route."""
import json

import pytest

from bloomsearch_amd import query as Q
from bloomsearch_amd.gpu import Context
from tests.test_engine_regex_substr_gpu import engine, found, make_rows, restated

pytestmark = pytest.mark.gpu

# three needles that are valid one by one and do not pack into 2 x 64 bytes (40 + 40 + 41), beside one that matches rows
NO_PACK = Q.SubstringOr(Q.Substring("10.0.3." + "z" * 33), Q.Substring("q" * 40), Q.Substring("reset by peer" + " " * 27 + "$"), Q.Substring("10.1.3."))
QUERIES = [
    (Q.FieldToken("level", "err"), None, None),                                          # bloom only
    (None, None, Q.Substring("10.0.3.")),                                                # substring only
    (Q.FieldToken("level", "err"), None, Q.SubstringOr(Q.Substring("reset by"), Q.Substring("cache"))),   # bloom + substring
    (None, Q.FieldRegex("msg", "timeout|cache"), Q.Substring("10.0.3.")),                # regex + substring
    (None, None, Q.FieldSubstring("msg", "TIMEOUT")),                                    # a FieldSubstring
    (None, None, NO_PACK),                                                               # alone beyond the packing: its single-query route
]
BATCHED = [0, 1, 2, 3, 4]
GROUP_CALLS = ("bsg_match_rows_many", "bsg_match_rows_many_regex", "bsg_match_rows_many_substr", "bsg_match_rows_many_regex_substr", "bsg_match_rows_wide",
               "bsg_match_rows_wide_rows", "bsg_match_rows_wide_substr", "bsg_match_rows_wide_substr_rows", "bsg_match_rows_lookup", "bsg_match_rows_lookup_rows")


@pytest.fixture(scope="module")
def rows():
    return make_rows()


@pytest.fixture(scope="module")
def want(rows):
    w = [restated(rows, *q) for q in QUERIES]
    assert all(w)                                # every query has rows to find
    assert len({json.dumps(x) for x in w}) == len(w)
    return w


def many(e, queries):
    res = e.query_many([q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries])
    assert len(res) == len(queries) and all(r["stats"]["Errors"] == [] for r in res)
    return [sorted(json.dumps(x, sort_keys=True) for x in r["rows"]) for r in res]


def test_the_batched_route(rows, want):
    with Context((0,)) as c:
        e = engine(c, rows, DeviceMatch=True, DeviceRegex=True)
        assert e.match_calls() == {}
        assert many(e, QUERIES) == want
        calls = e.match_calls()
        # queries 0-4 are ONE group with regex conditions and needles; query 5 took bsg_match_rows_substr by itself (refused there: the host)
        assert calls == {"bsg_match_rows_many_regex_substr": 1, "bsg_match_rows_substr": 1}, calls
        # without the one that does not pack nothing is left of the single-query calls
        assert many(e, [QUERIES[i] for i in BATCHED]) == [want[i] for i in BATCHED]
        after = e.match_calls()
        assert after == {"bsg_match_rows_many_regex_substr": 2, "bsg_match_rows_substr": 1}, after
        # ... and every answer is query()'s
        assert [found(e, *q) for q in QUERIES] == want
        e.close()


def test_a_group_without_a_regex_condition_takes_the_substring_call(rows, want):
    with Context((0,)) as c:
        e = engine(c, rows, DeviceMatch=True, DeviceRegex=True)
        keep = [0, 1, 2, 4]
        assert many(e, [QUERIES[i] for i in keep]) == [want[i] for i in keep]
        assert e.match_calls() == {"bsg_match_rows_many_substr": 1}
        e.close()
        # DeviceMatch without DeviceRegex: the regex query leaves the batch (query() decides it), the other four stay one group
        e = engine(c, rows, DeviceMatch=True)
        assert many(e, QUERIES) == want
        calls = e.match_calls()
        assert calls.get("bsg_match_rows_many_substr") == 1 and calls.get("bsg_match_rows_substr") == 1, calls
        assert not any(calls.get(name, 0) for name in GROUP_CALLS if name != "bsg_match_rows_many_substr"), calls
        assert calls.get("bsg_match_rows_regex_substr", 0) == 0
        e.close()


@pytest.mark.parametrize("key,call", [("DeviceMatchWide", "bsg_match_rows_wide_substr"), ("DeviceMatchWideRows", "bsg_match_rows_wide_substr_rows"),
                                      ("DeviceMatchLookup", "bsg_match_rows_wide_substr")])
def test_the_wide_route(rows, want, key, call):
    """under the wide keys the group calls the wide substring entry point; under a lookup key a group with a needle falls to the same"""
    with Context((0,)) as c:
        e = engine(c, rows, DeviceMatch=True, DeviceRegex=True, **{key: True})
        assert many(e, QUERIES) == want
        calls = e.match_calls()
        assert calls == {call: 1, "bsg_match_rows_substr": 1}, calls
        # a group without a needle keeps its call
        assert many(e, [QUERIES[0], QUERIES[0]]) == [want[0], want[0]]
        after = e.match_calls()
        plain = {"DeviceMatchWide": "bsg_match_rows_wide", "DeviceMatchWideRows": "bsg_match_rows_wide_rows", "DeviceMatchLookup": "bsg_match_rows_lookup"}[key]
        assert after == {call: 1, "bsg_match_rows_substr": 1, plain: 1}, after
        e.close()


def test_without_device_matching_nothing_is_called_and_the_answers_are_the_same(rows, want):
    with Context((0,)) as c:
        e = engine(c, rows)
        assert many(e, QUERIES) == want
        assert e.match_calls() == {}
        e.close()
