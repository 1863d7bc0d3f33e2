"""BloomSearchEngine::query_many under DeviceMatchLookupRegex: 200 queries on distinct tokens followed by 8 regex-only queries on
distinct fields.  With DeviceMatchLookupRows + DeviceRegex alone the first regex query closes the 200-condition lookup group and
opens a 64-condition one for the wide call: two match calls.  With DeviceMatchLookupRegex as well the batch stays one group of 208
conditions and is one bsg_match_rows_lookup_regex_rows call.  The answers equal those with every such key off: rows in the same
order, every BlockStats field but the duration, Errors, FilesConsidered, FilesBloomSkipped."""
import pytest

from bloomsearch_amd import query as Q
from tests.test_engine_query_many_gpu import build, comparable

pytestmark = pytest.mark.gpu

REGEX = [("id", "^1[0-9]$"), ("partition", "^p3$"), ("level", "^err"), ("service", "^pay"), ("message", "timeout|cache"), ("user.name", "(?i)^jo"),
         ("user.id", "^2$"), ("only6", "needle-[12]$")]


def test_regex_key_on_keeps_the_batch_in_one_match_call(ctx):
    exprs = [Q.Token(str(i)) for i in range(200)] + [None] * len(REGEX)                # ids of the rows, user ids, and numbers no row holds
    rxs = [None] * 200 + [Q.FieldRegex(f, p) for f, p in REGEX]
    off = build(ctx, DeviceMatch=True, DeviceRegex=True)
    two = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchLookupRows=True)
    one = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchLookupRows=True, DeviceMatchLookupRegex=True)
    bits = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchLookup=True, DeviceMatchLookupRegex=True)
    alone = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchLookupRegex=True)   # the key without a lookup key: today's grouping
    engines = (off, two, one, bits, alone)
    try:
        for e in engines:                                                              # arenas leased, tables warm: every side counted alike
            e.query_many(exprs, rxs)
        calls = []
        for e in (one, two, bits):
            c0 = ctx.device_calls().sum()
            got = e.query_many(exprs, rxs)
            calls.append((int(ctx.device_calls().sum() - c0), got))
        want = [comparable(x) for x in off.query_many(exprs, rxs)]
        for _, got in calls:
            assert [comparable(x) for x in got] == want
        assert [comparable(x) for x in alone.query_many(exprs, rxs)] == want
        got = calls[0][1]
        assert sum(len(x["rows"]) for x in got[:200]) > 400 and got[3]["rows"] and got[150]["rows"]
        assert all(got[200 + k]["rows"] for k in range(len(REGEX))) and all(r["service"].startswith("pay") for r in got[203]["rows"])
        # the grouping rule: a lookup group of 200 and a wide group of 8 against one group of 208
        assert calls[1][0] - calls[0][0] == 1 and calls[2][0] == calls[0][0]
        assert calls[0][0] <= calls[1][0]                                              # the key never makes more calls
    finally:
        for e in engines:
            e.close()
