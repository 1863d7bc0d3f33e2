"""BloomSearchEngine::query_many under DeviceMatchWide: the batch is packed into groups bounded by the condition table, not by 64
members, and each group is decided by one bsg_match_rows_wide call whose per-set query lists come straight from the probe's
survivors.  The answers equal those with the key off - rows in the same order, every BlockStats field but the duration, Errors,
FilesConsidered, FilesBloomSkipped - and the single queries', for 150 queries over at most 64 conditions with regex queries among
them, over three files, with rows the device hands back."""
import random

import pytest

from bloomsearch_amd import query as Q
from tests.test_engine_query_many_gpu import LEVELS, SERVICES, build, comparable

pytestmark = pytest.mark.gpu


def rx(field, pattern):
    return Q.FieldRegex(field, pattern)


def batch_of_150():
    r = random.Random(17)
    conds = ([Q.FieldToken("level", l) for l in LEVELS] + [Q.FieldToken("service", s) for s in SERVICES] +
             [Q.Token(w) for w in ("timeout", "retry", "cache", "miss", "ok", "disk", "full", "login", "failed")] +
             [Q.FieldToken("partition", "p%d" % i) for i in range(9)] + [Q.FieldToken("only6", "needle-%d" % i) for i in range(7)] +
             [Q.FieldToken("user.id", str(i)) for i in range(8)] + [Q.Field("user.name"), Q.Field("k" * 100), Q.FieldToken("user.name", "jane")])
    regexes = [rx("message", "timeout|cache"), rx("service", "^pay"), rx("level", "^err"), rx("user.name", "^j"), rx("k" * 100, "timeout")]
    assert len(conds) + len(regexes) <= 64
    exprs, rxs = [None, Q.And(), Q.Or(), Q.And(Q.Token("timeout"), Q.Field("k" * 100))], [None, None, None, None]   # the last one's rows are handed back
    while len(exprs) < 150:
        kind = len(exprs) % 5
        kids = r.sample(conds, r.randint(2, 4))
        exprs.append(Q.And(*kids[:2]) if kind in (0, 3) else Q.Or(*kids) if kind == 1 else Q.And(kids[0], Q.Or(*kids[1:])) if kind == 2 else r.choice(conds[:17]))
        rxs.append(r.choice(regexes) if len(exprs) % 12 == 0 else None)
    exprs[20], rxs[20] = None, Q.RegexAnd(rx("k" * 100, "timeout"), rx("level", "^err"))
    return exprs, rxs


def test_wide_key_on_equals_key_off(ctx):
    exprs, rxs = batch_of_150()
    assert sum(x is not None for x in rxs) >= 8
    off = build(ctx, DeviceMatch=True, DeviceRegex=True)
    on = build(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchWide=True)
    try:
        assert len(on.describe()["files"]) >= 2
        on.query_many(exprs, rxs)                                                      # arenas leased, tables warm: both sides measured alike
        off.query_many(exprs, rxs)
        c0 = ctx.device_calls().sum()
        got_on = on.query_many(exprs, rxs)
        c1 = ctx.device_calls().sum()
        got_off = off.query_many(exprs, rxs)
        c2 = ctx.device_calls().sum()
        assert [comparable(x) for x in got_on] == [comparable(x) for x in got_off]
        assert sum(len(x["rows"]) for x in got_on) > 3000 and got_on[3]["rows"] and got_on[20]["rows"]
        assert all("k" * 100 in r for r in got_on[3]["rows"])                          # decided by the host matcher: the path is longer than a lane keeps
        assert int(c1 - c0) < int(c2 - c1), (int(c1 - c0), int(c2 - c1))               # one match call for the batch against one per 64 queries
        for i in (0, 3, 7, 12, 20, 24, 77, 149):                                       # ... and the single queries answer the same
            assert comparable(on.query(exprs[i], rxs[i])) == comparable(got_on[i]), i
    finally:
        on.close()
        off.close()
