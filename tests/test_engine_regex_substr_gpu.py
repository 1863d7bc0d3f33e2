"""The engine mirror with a Regex tree AND a Substring tree in one query: under DeviceMatch + DeviceRegex ONE
bsg_match_rows_regex_substr call over And(bloom root, regex root, substring root) decides the scan list, and the engine answers as
one that decides on the host.  The expected rows come from the restatements (bloom: tests/ngram_restatement, regex: Python `re`
through test_match_regex_gpu.oracle_row, substring: tests/substring_restatement); Engine.match_calls() shows the route."""
import json
import re

import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd.gpu import Context
from tests import ngram_restatement as G
from tests import substring_restatement as SR
from tests.test_host_tables import go_marshal
from tests.test_match_regex_gpu import oracle_row
from tests.test_match_regex_substr_gpu import py_runner

pytestmark = pytest.mark.gpu

SPEC = SR.TRIGRAM
MSGS = {"p0": ["Connection reset by peer", "connection timeout", "all good"], "p1": ["request TIMEOUT", "timeout: cache cold", "fine"], "p2": ["ok", "idle loop"]}
COMBINED, OLD = "bsg_match_rows_regex_substr", ("bsg_match_rows_regex", "bsg_match_rows_tok", "bsg_match_rows_substr")


def make_rows():
    rows = []
    for i in range(300):
        p = "p%d" % (i % 3)
        rows.append({"id": i, "partition": p, "level": ["err", "inf"][(i // 3) % 2], "msg": MSGS[p][(i // 6) % len(MSGS[p])],
                     "peer": "10.0.3.%d" % i if i % 4 == 0 else "10.1.3.%d" % i})
    return [go_marshal(r) for r in rows]


QUERIES = [
    (None, Q.FieldRegex("msg", "timeout|cache"), Q.Substring("10.0.3.")),
    (Q.FieldToken("level", "err"), Q.RegexOr(Q.FieldRegex("msg", "timeout|retry"), Q.FieldRegex("level", "^err")), Q.FieldSubstring("peer", "10.0.3.")),
    (None, Q.FieldRegex("msg", "timeout|cache"), Q.SubstringOr(Q.FieldSubstring("msg", "TIMEOUT"), Q.Substring("reset by"))),
    (Q.Field("peer"), Q.FieldRegex("msg", "."), Q.SubstringAnd(Q.Substring("conn"), Q.FieldSubstring("peer", "10.1."))),
]

def restated(rows, bloom, rx, sx, runner=py_runner):
    return sorted(json.dumps(json.loads(r), sort_keys=True) for r in rows
                  if G.row_verdict(r, SPEC, bloom) and oracle_row(r, None, rx, runner) and SR.row_verdict(r, sx, SPEC))


def found(e, bloom, rx, sx):
    res = e.query(bloom, rx, sx)
    assert res["stats"]["Errors"] == []
    return sorted(json.dumps(x, sort_keys=True) for x in res["rows"])


def engine(c, rows, **kw):
    e = Hst.Engine(c, PartitionField="partition", MaxBufferedRows=1000, BloomFalsePositiveRate=0.0001, Tokenizer=SPEC, **kw)
    e.ingest_rows(rows)
    e.flush()
    return e


def test_engines_with_and_without_the_device_matchers_answer_alike():
    rows = make_rows()
    got = []
    for device in (False, True):
        with Context((0,)) as c:
            e = engine(c, rows, DeviceMatch=device, DeviceRegex=device)
            assert e.match_calls() == {}
            got.append([found(e, *q) for q in QUERIES])
            calls = e.match_calls()
            if device:
                # one combined call per query, and none of the calls the two sides took before
                assert calls.get(COMBINED) == len(QUERIES), calls
                assert all(calls.get(name, 0) == 0 for name in OLD), calls
            else:
                assert calls == {}
            e.close()
    assert got[0] == got[1]
    for i, q in enumerate(QUERIES):
        want = restated(rows, *q)
        assert got[1][i] == want and want, i
    assert len(QUERIES) == 4


def test_a_query_the_combined_call_does_not_hold_takes_the_parents_route():
    rows = make_rows()
    with Context((0,)) as c:
        e = engine(c, rows, DeviceMatch=True, DeviceRegex=True)
        # needles that are valid one by one but do not pack into 2 x 64 bytes: the library answers BSG_E_UNSUPPORTED, the regex call
        # decides bloom AND regex, the host the substring side
        sx = Q.SubstringOr(Q.Substring("10.0.3." + "z" * 33), Q.Substring("q" * 40), Q.Substring("reset by peer" + " " * 27 + "$"), Q.Substring("10.0.3."))
        q = (None, Q.FieldRegex("msg", "timeout|cache"), sx)
        assert found(e, *q) == restated(rows, *q) != []
        calls = e.match_calls()
        assert calls.get(COMBINED) == 1 and calls.get("bsg_match_rows_tok") == 1 and calls.get("bsg_match_rows_substr", 0) == 0, calls
        # a pattern outside the device subset: the old route from the start (the host's regex engine decides it)
        q = (None, Q.FieldRegex("msg", "\\btimeout"), Q.Substring("10.0.3."))
        assert found(e, *q) == restated(rows, *q, runner=lambda pattern, text: re.search(r"\btimeout", text) is not None) != []
        after = e.match_calls()
        assert after.get(COMBINED) == 1, after
        # DeviceMatch without DeviceRegex: no combined call either
        e.close()
        e = engine(c, rows, DeviceMatch=True, DeviceRegex=False)
        q = QUERIES[0]
        assert found(e, *q) == restated(rows, *q)
        assert COMBINED not in e.match_calls()
        e.close()
