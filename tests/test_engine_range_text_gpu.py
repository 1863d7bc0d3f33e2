"""The engine mirror's DeviceMatchRangeText key: under DeviceMatch, bse_query decides a query that has a Range tree beside a Regex and /
or a Substring tree by ONE bsg_match_rows_regex_substr_range call and returns the rows and block stats of the host-only engine; with
the key off every counted entry point is the one tests/test_engine_range_gpu.py pins.  The store is that file's: every sixteenth
row writes its timestamp with an exponent, so each case also hands rows back to the four host matchers."""
import json

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests.test_engine_range_gpu import RANGE, ROWS, engine, ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(ctx):
    host, off, on = engine(ctx), engine(ctx, DeviceMatch=True, DeviceRegex=True), engine(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchRangeText=True)
    yield host, off, on
    for e in (host, off, on):
        e.close()


# (query shape, the trees, the entry point counted with the key off)
SHAPES = [
    ("range + substring", {"substring_expression": Q.Substring("timeout")}, "bsg_match_rows_substr"),
    ("range + regex", {"regex_expression": Q.FieldRegex("msg", "timeout$")}, "bsg_match_rows_tok"),
    ("all three", {"regex_expression": Q.FieldRegex("lvl", "^err"), "substring_expression": Q.Substring("timeout")}, "bsg_match_rows_regex_substr"),
]
BLOOMS = [None, Q.FieldToken("lvl", "error")]


def grown(before, after):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def stats(res):
    return [(b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"]) for b in res["stats"]["BlockStats"]]


@pytest.mark.parametrize("bloom", range(len(BLOOMS)))
@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=[s[0].replace(" ", "_") for s in SHAPES])
def test_with_the_key_on_one_new_call_decides_the_query(engines, shape, bloom):
    host, off, on = engines
    _, kw, old_name = SHAPES[shape]
    b = BLOOMS[bloom]
    want = host.query(b, range_expression=RANGE, **kw)
    rx, sx = kw.get("regex_expression"), kw.get("substring_expression")
    assert ids(want) == [json.loads(r)["id"] for r in ROWS if Hst.match_row_range(RANGE, r) and (b is None or Hst.match_row(b, r)) and
                         (rx is None or Hst.match_row_regex(rx, r)) and (sx is None or Hst.match_row_substring(sx, r))]
    before = on.match_calls()
    got = on.query(b, range_expression=RANGE, **kw)
    assert grown(before, on.match_calls()) == {"bsg_match_rows_regex_substr_range": 1}
    assert ids(got) == ids(want) and stats(got) == stats(want)
    if bloom == 0:
        assert 0 < len(ids(got)) < len(ids(host.query(None, **kw)))
    # the key off: the entry point the parent commit counted, and the same rows
    before = off.match_calls()
    got = off.query(b, range_expression=RANGE, **kw)
    assert grown(before, off.match_calls()) == {old_name: 1} and ids(got) == ids(want) and stats(got) == stats(want)


def test_an_exponent_literal_in_the_store_is_decided_by_the_host_matchers(engines):
    host, off, on = engines
    rng = Q.FieldRange("ts", 1700000100, 1700000100)                             # 17000001e2 = 1700000100: rows that write it so are handed back
    sub = Q.Substring("request")
    want = ids(host.query(None, range_expression=rng, substring_expression=sub))
    assert want == [json.loads(r)["id"] for r in ROWS if Hst.match_row_range(rng, r)] and len(want) >= 2
    assert any(b'"ts":17000001e2' in ROWS[i] for i in want)
    before = on.match_calls()
    assert ids(on.query(None, range_expression=rng, substring_expression=sub)) == want
    assert grown(before, on.match_calls()) == {"bsg_match_rows_regex_substr_range": 1}


def test_the_key_changes_no_other_route(engines):
    """a Range tree alone, a text tree alone, a range tree beside nothing but a pattern outside the device subset: the calls of the engine
    without the key"""
    host, off, on = engines
    for kw in ({"range_expression": RANGE}, {"substring_expression": Q.Substring("timeout")}, {"regex_expression": Q.FieldRegex("msg", "timeout$")},
               {"regex_expression": Q.FieldRegex("lvl", "^err"), "substring_expression": Q.Substring("timeout")},
               {"range_expression": RANGE, "regex_expression": OUTSIDE}):
        b0, b1 = off.match_calls(), on.match_calls()
        a, b = off.query(None, **kw), on.query(None, **kw)
        assert grown(b0, off.match_calls()) == grown(b1, on.match_calls()) and NEW not in grown(b1, on.match_calls()), kw
        assert ids(a) == ids(b) == ids(host.query(None, **kw)), kw


NEW, NEW_MANY = "bsg_match_rows_regex_substr_range", "bsg_match_rows_many_regex_substr_range"
OUTSIDE = Q.FieldRegex("msg", "\\btimeout")                       # \b is outside the device subset: that tree stays on the host


def test_a_regex_tree_outside_the_subset_is_left_out_of_the_one_call(engines):
    """range and substring are decided in the one call, the host regex matcher filters its hits"""
    host, off, on = engines
    kw = {"range_expression": RANGE, "regex_expression": OUTSIDE, "substring_expression": Q.Substring("request")}
    want = host.query(None, **kw)
    before = on.match_calls()
    got = on.query(None, **kw)
    assert grown(before, on.match_calls()).get(NEW) == 1 and "bsg_match_rows_substr" not in grown(before, on.match_calls())
    assert ids(got) == ids(want) == ids(off.query(None, **kw)) and stats(got) == stats(want)
    assert 0 < len(ids(got)) < len(ids(host.query(None, range_expression=RANGE, substring_expression=Q.Substring("request"))))


def test_a_call_the_library_refuses_is_not_counted(engines):
    """three needles of 40 folded bytes do not pack: BSG_E_UNSUPPORTED, the route without the key, and only its calls are counted"""
    host, off, on = engines
    sub = Q.SubstringOr(Q.Substring("request " + "a" * 32), Q.Substring("request " + "b" * 32), Q.Substring("request " + "c" * 32), Q.Substring("timeout"))
    b0, b1 = off.match_calls(), on.match_calls()
    a, b = off.query(None, range_expression=RANGE, substring_expression=sub), on.query(None, range_expression=RANGE, substring_expression=sub)
    assert grown(b0, off.match_calls()) == grown(b1, on.match_calls()) and NEW not in grown(b1, on.match_calls())
    assert ids(a) == ids(b) == ids(host.query(None, range_expression=RANGE, substring_expression=sub)) and len(ids(a)) > 0


# (bloom, regex, substring, range): range only, text only, plain, and the three mixed shapes
MANY = [
    (None, None, None, RANGE), (Q.Token("request"), None, Q.Substring("served"), None), (Q.FieldToken("lvl", "error"), None, None, None),
    (None, None, Q.Substring("timeout"), RANGE), (None, Q.FieldRegex("msg", "timeout$"), None, RANGE),
    (Q.FieldToken("lvl", "error"), Q.FieldRegex("lvl", "^err"), Q.Substring("timeout"), RANGE),
    (None, Q.FieldRegex("lvl", "^err"), None, None), (None, None, Q.FieldSubstring("msg", "request 1"), Q.FieldRange("id", None, 150)),
]


def many(e, queries):
    return e.query_many([b for b, _, _, _ in queries], regex_expressions=[r for _, r, _, _ in queries], substring_expressions=[s for _, _, s, _ in queries],
                        range_expressions=[g for _, _, _, g in queries])


def single(e, quad):
    b, r, s, g = quad
    return e.query(b, regex_expression=r, substring_expression=s, range_expression=g)


def test_query_many_forms_one_mixed_group_and_answers_as_query(engines):
    host, off, on = engines
    want = [ids(single(host, quad)) for quad in MANY]
    assert all(len(w) > 0 for w in want)
    before = on.match_calls()
    got = many(on, MANY)
    assert grown(before, on.match_calls()) == {NEW_MANY: 1}                      # all eight queries in ONE group, one call
    assert [ids(r) for r in got] == want == [ids(single(on, quad)) for quad in MANY]
    for r, quad in zip(got, MANY):
        assert stats(r) == stats(single(host, quad))
    # the key off: the mixed queries go to query() one by one, the others form the groups they formed
    before = off.match_calls()
    got = many(off, MANY)
    g = grown(before, off.match_calls())
    assert NEW_MANY not in g and NEW not in g and sum(g.values()) > 1 and [ids(r) for r in got] == want
    # a range-only and a text-only query share a group under the key (two groups without it); range-only and plain ones keep their call
    assert grown_of(on, MANY[:2]) == {NEW_MANY: 1} and grown_of(off, MANY[:2]) == {"bsg_match_rows_many_range": 1, "bsg_match_rows_many_substr": 1}
    assert grown_of(on, [MANY[0], MANY[2]]) == grown_of(off, [MANY[0], MANY[2]]) == {"bsg_match_rows_many_range": 1}


def grown_of(e, queries):
    before = e.match_calls()
    many(e, queries)
    return grown(before, e.match_calls())


def counted(n):
    return "^[0-9a-f]{%d}$" % n                              # a DFA of n + 2 states: 4 n + 290 bytes of table with its user mask


def four_tables(tag, n0):
    """Or(timeout$ on msg, four counted patterns on four fields of their own): about 4 * (4 n0 + 290) bytes of regex tables"""
    return Q.RegexOr(Q.FieldRegex("msg", "timeout$"), *[Q.FieldRegex("%s%d" % (tag, i), counted(n0 + i)) for i in range(4)])


def test_a_mixed_group_that_would_pass_34032_bytes_closes(engines):
    """eight regex tables of 34 112 bytes in all (and timeout$'s) fit bsg_match_rows_many_regex's 38 140 bytes, not the 34 032 a table
    with kind 6 beside a text condition has, needle or not: the second query opens a second group.  At 31 232 bytes they share one."""
    host, off, on = engines
    big = [(None, four_tables("fa", 990), None, RANGE), (None, four_tables("fb", 994), None, RANGE)]
    want = [ids(single(host, quad)) for quad in big]
    assert len(want[0]) > 0 and want[0] == want[1]
    before = on.match_calls()
    got = many(on, big)
    assert grown(before, on.match_calls()) == {NEW_MANY: 2} and [ids(r) for r in got] == want
    # the same tables without the range trees: one group of the batched regex call
    assert grown_of(on, [(b, r, s, None) for b, r, s, _ in big]) == {"bsg_match_rows_many_regex": 1}
    # under the cap: one mixed group
    small = [(None, four_tables("fa", 900), None, RANGE), (None, four_tables("fb", 904), None, RANGE)]
    before = on.match_calls()
    got = many(on, small)
    assert grown(before, on.match_calls()) == {NEW_MANY: 1} and [ids(r) for r in got] == want


def test_under_a_wide_key_groups_never_mix(ctx):
    e = engine(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchRangeText=True, DeviceMatchWide=True)
    try:
        before = e.match_calls()
        got = many(e, MANY)
        g = grown(before, e.match_calls())
        assert NEW_MANY not in g and g.get(NEW, 0) == 4                           # the four mixed queries: query(), where the key applies
        host = engine(ctx)
        try:
            assert [ids(r) for r in got] == [ids(single(host, quad)) for quad in MANY]
        finally:
            host.close()
    finally:
        e.close()
