"""BloomSearchEngine::query_many under DeviceMatchLookupRows: a batch of 200 queries on distinct tokens is one group of 200 conditions
and one bsg_match_rows_lookup_rows call, where DeviceMatchWideRows cuts it into four groups of at most 64 conditions.  The answers
equal those with every such key off: rows in the same order, every BlockStats field but the duration, Errors, FilesConsidered,
FilesBloomSkipped."""
import pytest

from bloomsearch_amd import query as Q
from tests.test_engine_query_many_gpu import build, comparable

pytestmark = pytest.mark.gpu


def test_lookup_rows_key_on_equals_key_off_in_one_match_call(ctx):
    exprs = [Q.Token(str(i)) for i in range(200)]                                      # ids of the rows, user ids, and numbers no row holds
    rxs = [None] * len(exprs)
    off = build(ctx, DeviceMatch=True)
    wide = build(ctx, DeviceMatch=True, DeviceMatchWideRows=True)
    lookup = build(ctx, DeviceMatch=True, DeviceMatchLookupRows=True)
    bits = build(ctx, DeviceMatch=True, DeviceMatchLookup=True)
    try:
        for e in (off, wide, lookup, bits):                                            # arenas leased, tables warm: every side counted alike
            e.query_many(exprs, rxs)
        c0 = ctx.device_calls().sum()
        got_lookup = lookup.query_many(exprs, rxs)
        c1 = ctx.device_calls().sum()
        got_wide = wide.query_many(exprs, rxs)
        c2 = ctx.device_calls().sum()
        got_bits = bits.query_many(exprs, rxs)
        c3 = ctx.device_calls().sum()
        got_off = off.query_many(exprs, rxs)
        want = [comparable(x) for x in got_off]
        assert [comparable(x) for x in got_lookup] == want and [comparable(x) for x in got_wide] == want and [comparable(x) for x in got_bits] == want
        assert sum(len(x["rows"]) for x in got_lookup) > 400 and got_lookup[3]["rows"] and got_lookup[150]["rows"]
        assert int(c2 - c1) - int(c1 - c0) == 3                                        # four wide match calls (64 + 64 + 64 + 8 conditions) against one
        assert int(c3 - c2) == int(c1 - c0)
    finally:
        for e in (off, wide, lookup, bits):
            e.close()
