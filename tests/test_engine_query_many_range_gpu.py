"""The engine mirror's query_many with Range trees: under DeviceMatch a query with a Range tree and neither a Regex nor a Substring
tree stays in the batch's groups, and a group with a range condition is decided by ONE bsg_match_rows_many_range call — under the
wide keys (and the lookup keys, which never take such a group) by ONE bsg_match_rows_wide_range(_rows) call — instead of one
bsg_match_rows_range call per query.  Every answer is the host-only engine's; Engine.match_calls() shows the route."""
import itertools

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests.test_engine_range_gpu import RANGE, ROWS, engine, ids

pytestmark = pytest.mark.gpu

POINT = Q.FieldRange("ts", 1700000100, 1700000100)       # row 100, and the seven rows that write 17000001e2
# (bloom, regex, substring, range)
QUERIES = [
    (Q.FieldToken("lvl", "error"), None, None, None),                                    # plain
    (Q.Token("timeout"), None, None, None),
    (None, None, None, RANGE),                                                           # range only
    (Q.FieldToken("lvl", "error"), None, None, RANGE),                                   # range + bloom
    (Q.Token("timeout"), None, None, Q.RangeOr(Q.FieldRange("ts", None, 1700000020), Q.FieldRange("id", 300, None))),
    (None, None, None, POINT),                                                           # an exponent literal among its rows
    (None, Q.FieldRegex("msg", "timeout$"), None, RANGE),                                # range + regex: query()'s route
    (None, None, Q.Substring("timeout"), RANGE),                                         # range + substring: the same
]
BATCHED, MIXED = [0, 1, 2, 3, 4, 5], [6, 7]
MIXED_CALLS = {"bsg_match_rows_tok": 1, "bsg_match_rows_substr": 1}                     # what query() counts for the two (tests/test_engine_range_gpu.py)
# seventy (bloom, range) queries over 17 distinct conditions
BLOOMS = [None, Q.FieldToken("lvl", "error"), Q.FieldToken("lvl", "info"), Q.Token("timeout"), Q.Token("served"), Q.Field("ts"), Q.Token("request"),
          Q.FieldToken("partition", "a"), Q.FieldToken("partition", "b"), Q.And(Q.Token("request"), Q.Field("ts"))]
RANGES = [RANGE, POINT, Q.FieldRange("id", 17, 17), Q.FieldRange("ts", None, 1700000040, hi_open=True), Q.FieldRange("id", 250, None, lo_open=True),
          Q.FieldRange("ts", 1700000300, 1700000200), Q.RangeAnd(RANGE, Q.FieldRange("id", 100, 160))]
SEVENTY = [(b, None, None, g) for b, g in itertools.product(BLOOMS, RANGES)]


def many(e, queries):
    res = e.query_many([q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries], [q[3] for q in queries])
    assert len(res) == len(queries) and all(r["stats"]["Errors"] == [] for r in res)
    return [ids(r) for r in res]


def grown(e, before):
    return {k: v - before.get(k, 0) for k, v in e.match_calls().items() if v != before.get(k, 0)}


@pytest.fixture(scope="module")
def want(ctx):
    host = engine(ctx)
    w = {"queries": many(host, QUERIES), "seventy": many(host, SEVENTY)}
    # without DeviceMatch query_many makes the calls it makes today: none
    assert host.match_calls() == {}
    host.close()
    for (bloom, rx, sx, rng), got in zip(QUERIES, w["queries"]):
        if rx is None and sx is None:
            assert got == [i for i, r in enumerate(ROWS) if Hst.match_row_range(rng, r) and (bloom is None or Hst.match_row(bloom, r))]
    assert all(w["queries"]) and {17, 65, 100} <= set(w["queries"][5]) and len(w["queries"][5]) == 8
    assert sum(bool(x) for x in w["seventy"]) > 40 and not all(w["seventy"])
    return w


def test_the_batched_route(ctx, want):
    e = engine(ctx, DeviceMatch=True, DeviceRegex=True)
    assert e.match_calls() == {}
    assert many(e, QUERIES) == want["queries"]
    # queries 0-5 are ONE group with range conditions; the two with another tree beside the range tree took query()'s route
    assert e.match_calls() == {"bsg_match_rows_many_range": 1, **MIXED_CALLS}
    before = e.match_calls()
    assert many(e, [QUERIES[i] for i in BATCHED]) == [want["queries"][i] for i in BATCHED]
    assert grown(e, before) == {"bsg_match_rows_many_range": 1}                        # and no bsg_match_rows_range call
    # seventy range queries: two groups of the batched call
    before = e.match_calls()
    assert many(e, SEVENTY) == want["seventy"]
    assert grown(e, before) == {"bsg_match_rows_many_range": 2}
    # a group closes where a range condition would meet a regex condition, in either order; plain queries go with both
    before = e.match_calls()
    regex = (None, Q.FieldRegex("msg", "timeout|served"), None, None)
    order = [QUERIES[2], QUERIES[0], regex, QUERIES[1], QUERIES[3], QUERIES[5]]
    got = many(e, order)
    assert got[:2] + got[3:] == [want["queries"][i] for i in (2, 0, 1, 3, 5)] and len(got[2]) == len(ROWS)
    assert grown(e, before) == {"bsg_match_rows_many_range": 2, "bsg_match_rows_many_regex": 1}
    # every answer is query()'s, one bsg_match_rows_range call each
    before = e.match_calls()
    assert [ids(e.query(q[0], range_expression=q[3])) for q in QUERIES[2:6]] == want["queries"][2:6]
    assert grown(e, before) == {"bsg_match_rows_range": 4}
    e.close()


def test_device_match_without_device_regex(ctx, want):
    e = engine(ctx, DeviceMatch=True)
    assert many(e, QUERIES) == want["queries"]
    calls = e.match_calls()
    assert calls.get("bsg_match_rows_many_range") == 1 and "bsg_match_rows_range" not in calls, calls
    e.close()


@pytest.mark.parametrize("key,call,plain", [("DeviceMatchWide", "bsg_match_rows_wide_range", "bsg_match_rows_wide"),
                                            ("DeviceMatchWideRows", "bsg_match_rows_wide_range_rows", "bsg_match_rows_wide_rows"),
                                            ("DeviceMatchLookup", "bsg_match_rows_wide_range", "bsg_match_rows_lookup"),
                                            ("DeviceMatchLookupRows", "bsg_match_rows_wide_range_rows", "bsg_match_rows_lookup_rows")])
def test_the_wide_routes_and_the_lookup_keys(ctx, want, key, call, plain):
    """under the wide keys a group with a range condition calls the wide range entry point; under a lookup key it falls to the same,
    and a group without one still takes the lookup call"""
    e = engine(ctx, DeviceMatch=True, DeviceRegex=True, **{key: True})
    assert many(e, QUERIES) == want["queries"]
    assert e.match_calls() == {call: 1, **MIXED_CALLS}
    # more than 64 range queries are one group, hence one call
    before = e.match_calls()
    assert many(e, SEVENTY) == want["seventy"]
    assert grown(e, before) == {call: 1}
    # a group without a range condition keeps its call
    before = e.match_calls()
    assert many(e, [QUERIES[0], QUERIES[1]]) == want["queries"][:2]
    assert grown(e, before) == {plain: 1}
    e.close()


def test_without_device_matching_nothing_is_called_and_the_answers_are_the_same(ctx, want):
    e = engine(ctx)
    assert many(e, QUERIES) == want["queries"]
    assert e.match_calls() == {}
    e.close()
