"""The engine mirror with a Range tree: the range guard prunes, and under DeviceMatch a query with neither a Regex nor a Substring tree
is decided by ONE bsg_match_rows_range call; every route returns the rows the host-only engine returns."""
import json

import pytest

from bloomsearch_amd import host as Hst, query as Q

pytestmark = pytest.mark.gpu

PARTS = ["a", "b", "c", "d"]


def make_rows():
    """320 rows over four partitions (one block each); no row of partition d has a timestamp, and every sixteenth row (all in
    partition b) writes its timestamp with an exponent: 17000001e0, e1 or e2"""
    out = []
    for i in range(320):
        p = PARTS[i % 4]
        ts = "" if p == "d" else ',"ts":%s' % ("17000001e%d" % (i % 3) if i % 16 == 1 else str(1700000000 + i))
        out.append(('{"id":%d,"partition":"%s","lvl":"%s","msg":"request %d %s"%s}' % (i, p, "error" if i % 5 == 0 else "info", i, "timeout" if i % 7 == 0 else "served", ts)).encode())
    return out


ROWS = make_rows()


def engine(ctx, **cfg):
    e = Hst.Engine(ctx, PartitionField="partition", BloomFalsePositiveRate=1e-6, MaxBufferedRows=100000, **cfg)
    e.ingest_rows(ROWS)
    e.flush()
    return e


@pytest.fixture(scope="module")
def engines(ctx):
    host, dev = engine(ctx), engine(ctx, DeviceMatch=True, DeviceRegex=True)
    yield host, dev
    host.close()
    dev.close()


def ids(res):
    return sorted(r["id"] for r in res["rows"])


RANGE = Q.FieldRange("ts", 1700000050, 1700000200, hi_open=True)
CASES = [
    (None, RANGE), (Q.FieldToken("lvl", "error"), RANGE), (Q.Token("timeout"), Q.RangeOr(Q.FieldRange("ts", None, 1700000020), Q.FieldRange("id", 300, None))),
    (None, Q.FieldRange("ts", 170000010, 170000010)), (None, Q.FieldRange("ts", 1700000100, 1700000100)), (Q.Field("ts"), Q.FieldRange("id", 17, 17)),
]


def test_the_rows_hold_what_the_cases_need():
    assert sum(b'"ts":17000001e' in r for r in ROWS) == 20 and sum(b'"ts"' not in r for r in ROWS) == 80
    assert all(json.loads(r)["id"] == i for i, r in enumerate(ROWS))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_match_returns_the_host_engines_rows_in_one_range_call(engines, case):
    host, dev = engines
    bloom, rng = CASES[case]
    want = host.query(bloom, range_expression=rng)
    assert ids(want) == [json.loads(r)["id"] for r in ROWS if Hst.match_row_range(rng, r) and (bloom is None or Hst.match_row(bloom, r))]
    before = dev.match_calls()
    got = dev.query(bloom, range_expression=rng)
    after = dev.match_calls()
    assert ids(got) == ids(want)
    assert [(b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"]) for b in got["stats"]["BlockStats"]] == \
        [(b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"]) for b in want["stats"]["BlockStats"]]
    grown = {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}
    assert grown == {"bsg_match_rows_range": 1}
    if case == 0:
        assert len(ids(got)) > 50 and host.match_calls() == {}


def test_an_exponent_literal_in_the_store_is_decided_by_the_host_matcher(engines):
    host, dev = engines
    rng = Q.FieldRange("ts", 1700000100, 1700000100)                             # 17000001e2 = 1700000100: two rows hold that value
    assert ids(dev.query(None, range_expression=rng)) == ids(host.query(None, range_expression=rng))
    assert len(ids(dev.query(None, range_expression=rng))) >= 2


def test_with_a_regex_or_substring_tree_the_existing_entry_point_is_counted(engines):
    host, dev = engines
    for kw, name in (({"regex_expression": Q.FieldRegex("msg", "timeout$")}, "bsg_match_rows_tok"), ({"substring_expression": Q.Substring("timeout")}, "bsg_match_rows_substr"),
                     ({"regex_expression": Q.FieldRegex("lvl", "^err"), "substring_expression": Q.Substring("timeout")}, "bsg_match_rows_regex_substr")):
        want = host.query(None, range_expression=RANGE, **kw)
        before = dev.match_calls()
        got = dev.query(None, range_expression=RANGE, **kw)
        after = dev.match_calls()
        assert ids(got) == ids(want) and 0 < len(ids(got)) < len(ids(host.query(None, **kw)))
        grown = {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}
        assert grown == {name: 1}


def test_query_many_answers_range_queries_as_query_does(engines):
    host, dev = engines
    blooms = [c[0] for c in CASES] + [Q.Token("timeout"), None]
    ranges = [c[1] for c in CASES] + [None, None]
    for e in (host, dev):
        many = e.query_many(blooms, range_expressions=ranges)
        assert [ids(r) for r in many] == [ids(e.query(b, range_expression=g)) for b, g in zip(blooms, ranges)]
    assert [ids(r) for r in dev.query_many(blooms, range_expressions=ranges)] == [ids(r) for r in host.query_many(blooms, range_expressions=ranges)]


def test_a_block_whose_rows_lack_the_field_is_pruned_by_the_field_guard(engines):
    for e in engines:
        res = e.query(None, range_expression=Q.FieldRange("ts", None, None))
        stats = res["stats"]["BlockStats"]
        assert len(stats) == 4 and sum(b["BloomFilterSkipped"] for b in stats) == 1
        skipped = [b for b in stats if b["BloomFilterSkipped"]][0]
        assert skipped["RowsProcessed"] == 0 and skipped["TotalRows"] == 80
        assert not any(json.loads(r)["partition"] == "d" for r in map(json.dumps, res["rows"]))
        assert Hst.prune_query_range(None, None, None, Q.FieldRange("ts", None, None)) == Q.Field("ts")
        assert sum(b["BloomFilterSkipped"] for b in e.query(None)["stats"]["BlockStats"]) == 0
