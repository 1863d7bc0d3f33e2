"""The engine mirror with a Substring tree in the query: files and blocks are pruned with And(bloom, regex guard, substring guard),
rows are decided exactly, and an engine with DeviceMatch (one bsg_match_rows_substr call per query) answers like one without."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd.gpu import Context
from tests import ngram_restatement as G
from tests import substring_restatement as SR
from tests.test_host_tables import go_marshal

pytestmark = pytest.mark.gpu

SPEC = SR.TRIGRAM
# three partitions = three blocks of one file: p0 has the resets, p1 the timeouts, p2 neither
MSGS = {"p0": ["Connection reset by peer", "connection reset", "all good"], "p1": ["request TIMEOUT", "Timeout: lock", "fine"], "p2": ["ok", "idle loop"]}


def make_rows():
    rows = []
    for i in range(300):
        p = "p%d" % (i % 3)
        rows.append({"id": i, "partition": p, "level": ["err", "inf"][(i // 3) % 2], "msg": MSGS[p][(i // 6) % len(MSGS[p])],
                     "note": "reset by %d" % i if i % 50 == 2 else "n/a"})
    return [go_marshal(r) for r in rows]


QUERIES = [
    (None, Q.Substring("ction res")),
    (None, Q.FieldSubstring("msg", "TIMEOUT")),
    (None, Q.SubstringOr(Q.Substring("by"), Q.FieldSubstring("msg", "timeout"))),          # "by" alone gives no term: the Or prunes nothing
    (Q.FieldToken("level", "err"), Q.SubstringAnd(Q.Substring("reset"), Q.FieldSubstring("msg", "conn"))),
]


def answers(e):
    out = []
    for bloom, sub in QUERIES:
        res = e.query(bloom, None, sub)
        assert res["stats"]["Errors"] == []
        out.append((sorted(json.dumps(x, sort_keys=True) for x in res["rows"]),
                    [(b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"]) for b in res["stats"]["BlockStats"]]))
    return out


def test_both_engines_answer_alike_and_prune_with_the_windows():
    rows = make_rows()
    got, calls = [], []
    for device in (False, True):
        with Context((0,)) as c:
            e = Hst.Engine(c, PartitionField="partition", MaxBufferedRows=1000, BloomFalsePositiveRate=0.0001, Tokenizer=SPEC, DeviceMatch=device)
            e.ingest_rows(rows)
            e.flush()
            assert [len(f["blocks"]) for f in e.describe()["files"]] == [3]
            before = int(c.device_calls().sum())
            got.append(answers(e))
            calls.append(int(c.device_calls().sum()) - before)
            many = e.query_many([b for b, _ in QUERIES], None, [s for _, s in QUERIES])       # a substring query in a batch: as bse_query
            assert [sorted(json.dumps(x, sort_keys=True) for x in m["rows"]) for m in many] == [a[0] for a in got[-1]]
            e.close()
    assert got[0] == got[1]
    # bsg_device_calls counts the probe's parts in both engines; with DeviceMatch each query adds its ONE bsg_match_rows_substr part
    assert calls[1] == calls[0] + len(QUERIES), calls
    for (bloom, sub), (found, stats) in zip(QUERIES, got[1]):
        want = sorted(json.dumps(json.loads(r), sort_keys=True) for r in rows if SR.row_verdict(r, sub, SPEC) and G.row_verdict(r, SPEC, bloom))
        assert found == want and want
    skipped = [[s[1] for s in stats] for _, stats in got[1]]           # blocks in partition order p0, p1, p2
    assert skipped[0] == [False, True, True]                           # only p0 holds the windows of "ction" and "res"
    assert skipped[1] == [True, False, True]
    assert skipped[2] == [False, False, False]                         # the termless child keeps every block
    assert skipped[3] == [False, True, True]


def test_a_needle_outside_the_limits_is_an_invalid_query():
    with Context((0,)) as c:
        e = Hst.Engine(c, Tokenizer=SPEC, DeviceMatch=True)
        e.ingest_rows([b'{"msg":"x"}'])
        e.flush()
        for bad in ("", "x" * 65):
            with pytest.raises(Hst.HostError):
                e.query(None, None, Q.Substring(bad))
        assert e.query(None, None, Q.Substring("x" * 64))["rows"] == []
        e.close()
