"""The engine mirror's DeviceMatchRangeTextWide key: under DeviceMatch, DeviceMatchRangeText and a wide or lookup key, bse_query_many lets
range conditions and text conditions share a WIDE group, decided by ONE bsg_match_rows_wide_regex_substr_range(_rows) call, and
returns the rows and block stats of the host-only engine; without the key every counted entry point is the one
tests/test_engine_range_text_gpu.py pins.  The store is tests/test_engine_range_gpu.py's: every sixteenth row writes its timestamp
with an exponent, so the batches also hand rows back to the four host matchers."""
import itertools

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests.test_engine_range_gpu import RANGE, engine, ids
from tests.test_engine_range_text_gpu import MANY, NEW, NEW_MANY, OUTSIDE, four_tables, grown, many, single, stats

pytestmark = pytest.mark.gpu

NEW_WIDE, NEW_WIDE_ROWS = "bsg_match_rows_wide_regex_substr_range", "bsg_match_rows_wide_regex_substr_range_rows"
BASE = dict(DeviceMatch=True, DeviceRegex=True, DeviceMatchRangeText=True)


@pytest.fixture(scope="module")
def host(ctx):
    e = engine(ctx)
    yield e
    e.close()


@pytest.fixture(scope="module")
def wide(ctx):
    e = engine(ctx, DeviceMatchRangeTextWide=True, DeviceMatchWide=True, **BASE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def want_many(host):
    return [single(host, quad) for quad in MANY]


@pytest.mark.parametrize("key,name", [("DeviceMatchWide", NEW_WIDE), ("DeviceMatchWideRows", NEW_WIDE_ROWS), ("DeviceMatchLookup", NEW_WIDE),
                                      ("DeviceMatchLookupRows", NEW_WIDE_ROWS)])
def test_one_new_call_decides_the_mixed_batch(ctx, want_many, key, name):
    e = engine(ctx, DeviceMatchRangeTextWide=True, **{key: True}, **BASE)
    try:
        before = e.match_calls()
        got = many(e, MANY)
        assert grown(before, e.match_calls()) == {name: 1}                          # all eight queries in ONE wide group, one call
        assert [ids(r) for r in got] == [ids(w) for w in want_many] and all(len(ids(w)) > 0 for w in want_many)
        assert [stats(r) for r in got] == [stats(w) for w in want_many]
        # bse_query is unchanged: the single call of DeviceMatchRangeText
        before = e.match_calls()
        assert ids(single(e, MANY[3])) == ids(want_many[3]) and grown(before, e.match_calls()) == {NEW: 1}
    finally:
        e.close()


def test_without_the_key_groups_never_mix_under_a_wide_key(ctx, want_many):
    """what tests/test_engine_range_text_gpu.py::test_under_a_wide_key_groups_never_mix states"""
    e = engine(ctx, DeviceMatchWide=True, **BASE)
    try:
        before = e.match_calls()
        got = many(e, MANY)
        g = grown(before, e.match_calls())
        assert NEW_MANY not in g and NEW_WIDE not in g and NEW_WIDE_ROWS not in g and g.get(NEW, 0) == 4
        assert [ids(r) for r in got] == [ids(w) for w in want_many]
    finally:
        e.close()


def test_seventy_mixed_queries_that_share_conditions_form_one_group(host, wide):
    regexes = [None, Q.FieldRegex("msg", "timeout$"), Q.FieldRegex("lvl", "^err")]
    subs = [None, Q.Substring("timeout"), Q.FieldSubstring("msg", "request 1")]
    ranges = [RANGE, Q.FieldRange("id", None, 150), Q.FieldRange("ts", 1700000100, None), Q.FieldRange("id", 40, 250, lo_open=True), Q.FieldRange("ts", None, 1700000150, hi_open=True),
              Q.FieldRange("id", 7, 7), Q.FieldRange("ts", 1700000100, 1700000100), Q.FieldRange("id", 100, None)]
    queries = [(Q.FieldToken("lvl", "error") if i % 9 == 0 else None, r, s, g) for i, (r, s, g) in enumerate(itertools.product(regexes, subs, ranges))][2:]
    assert len(queries) == 70 and sum(1 for _, r, s, _ in queries if r or s) > 50
    before = wide.match_calls()
    got = many(wide, queries)
    assert grown(before, wide.match_calls()) == {NEW_WIDE: 1}                        # more members than a batched call holds
    want = [single(host, quad) for quad in queries]
    assert [ids(r) for r in got] == [ids(w) for w in want] and sum(len(ids(w)) > 0 for w in want) > 30
    assert [stats(r) for r in got] == [stats(w) for w in want]


def test_a_mixed_wide_group_that_would_pass_42496_bytes_closes(host, wide):
    """eight counted tables of 33 944 bytes and timeout$'s in the first query; four more of about 9 500 bytes pass the 42 496 a wide table
    with kind 6 beside a text condition has, needle or not, and the second query opens a second group; four of about 7 250 share it"""
    first = (None, Q.RegexOr(four_tables("fa", 990), four_tables("fb", 990)), None, RANGE)
    big = [first, (None, four_tables("fc", 520), None, RANGE)]
    want = [ids(single(host, quad)) for quad in big]
    assert len(want[0]) > 0 and want[0] == want[1]
    before = wide.match_calls()
    got = many(wide, big)
    assert grown(before, wide.match_calls()) == {NEW_WIDE: 2} and [ids(r) for r in got] == want
    small = [first, (None, four_tables("fc", 380), None, RANGE)]
    before = wide.match_calls()
    got = many(wide, small)
    assert grown(before, wide.match_calls()) == {NEW_WIDE: 1} and [ids(r) for r in got] == want
    # the same tables without the range trees are under the wide call's own 46 592 bytes: one group
    before = wide.match_calls()
    many(wide, [(b, r, s, None) for b, r, s, _ in big])
    assert grown(before, wide.match_calls()) == {"bsg_match_rows_wide": 1}


def test_an_exponent_literal_in_the_store_is_decided_by_the_host_matchers(host, wide):
    rng = Q.FieldRange("ts", 1700000100, 1700000100)                             # 17000001e2 = 1700000100: rows that write it so are handed back
    queries = [(None, None, Q.Substring("request"), rng), (None, Q.FieldRegex("lvl", "^inf"), None, rng)]
    want = [ids(single(host, quad)) for quad in queries]
    assert len(want[0]) >= 2
    before = wide.match_calls()
    got = many(wide, queries)
    assert grown(before, wide.match_calls()) == {NEW_WIDE: 1} and [ids(r) for r in got] == want


def test_a_pattern_outside_the_device_subset_sends_only_its_own_query_to_query(host, wide):
    outside = (None, OUTSIDE, None, RANGE)
    before = wide.match_calls()
    single(wide, outside)
    alone = grown(before, wide.match_calls())
    assert NEW_WIDE not in alone
    queries = [MANY[3], outside, MANY[4], MANY[5]]
    before = wide.match_calls()
    got = many(wide, queries)
    g = grown(before, wide.match_calls())
    assert g.pop(NEW_WIDE) == 1 and g == alone                                   # the other three: one group, one call
    assert [ids(r) for r in got] == [ids(single(host, quad)) for quad in queries]


@pytest.mark.parametrize("cfg", [dict(DeviceMatchRangeText=True, DeviceMatchWide=True), dict(DeviceMatch=True, DeviceMatchWide=True),
                                 dict(DeviceMatch=True, DeviceMatchRangeText=True), dict()])
def test_the_key_without_its_prerequisites_is_refused_at_open(ctx, cfg):
    with pytest.raises(Hst.HostError) as e:
        Hst.Engine(ctx, DeviceMatchRangeTextWide=True, **cfg)
    assert e.value.code == -101
    # ... and each prerequisite set opens
    Hst.Engine(ctx, DeviceMatchRangeTextWide=True, DeviceMatch=True, DeviceMatchRangeText=True, DeviceMatchLookupRows=True).close()
