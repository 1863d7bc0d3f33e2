"""BloomSearchEngine::query_many under DeviceMatchWideRows: the groups of DeviceMatchWide, each decided by one bsg_match_rows_wide_rows
call whose tagged row lists are consumed as they come.  The answers equal those with the key off and those under DeviceMatchWide -
rows in the same order, every BlockStats field but the duration, Errors, FilesConsidered, FilesBloomSkipped - and the single
queries', for the 150 queries of the wide engine test: regex queries among them, three files, rows the device hands back."""
import pytest

from tests.test_engine_query_many_gpu import build, comparable
from tests.test_engine_query_many_wide_gpu import batch_of_150

pytestmark = pytest.mark.gpu


def test_rows_key_on_equals_key_off(ctx):
    exprs, rxs = batch_of_150()
    off = build(ctx, DeviceMatch=True, DeviceRegex=True)
    wide = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchWide=True)
    on = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchWideRows=True)
    try:
        assert len(on.describe()["files"]) >= 2
        on.query_many(exprs, rxs)                                                      # arenas leased, tables warm
        off.query_many(exprs, rxs)
        c0 = ctx.device_calls().sum()
        got_on = on.query_many(exprs, rxs)
        c1 = ctx.device_calls().sum()
        got_off = off.query_many(exprs, rxs)
        c2 = ctx.device_calls().sum()
        assert [comparable(x) for x in got_on] == [comparable(x) for x in got_off]
        assert [comparable(x) for x in got_on] == [comparable(x) for x in wide.query_many(exprs, rxs)]
        assert sum(len(x["rows"]) for x in got_on) > 3000 and got_on[3]["rows"] and got_on[20]["rows"]
        assert all("k" * 100 in r for r in got_on[3]["rows"])                          # decided by the host matcher: handed back by the list call too
        assert int(c1 - c0) < int(c2 - c1), (int(c1 - c0), int(c2 - c1))               # one match call for the batch, as under DeviceMatchWide
        for i in (0, 3, 7, 20, 77, 149):                                               # ... and the single queries answer the same
            assert comparable(on.query(exprs[i], rxs[i])) == comparable(got_on[i]), i
    finally:
        on.close()
        wide.close()
        off.close()
