"""The engine mirror with a "Tokenizer" of the separator family: Token("alice") finds {"msg":"user=alice"}, the default
engine does not; and with DeviceIngest / DeviceMatch / DeviceRegex on and off the rows, BlockStats and the filters bse_describe
reports are identical, through flushes and a merge."""
import json
import random

import pytest

from bloomsearch_amd import host as Hst
from bloomsearch_amd.gpu import Context
from tests import tokenizer_restatement as R
from tests.test_host_tables import go_marshal

pytestmark = pytest.mark.gpu

WORDS = ["user=alice", "user=bob", "GET /api/v1/users", "error:timeout", "retry", "Cache-Miss", "db.shard", "ok", "K=v", "a,b;c"]


def make_rows(seed, n):
    r = random.Random(seed)
    rows = []
    for i in range(n):
        row = {"id": i, "partition": "p%d" % (i % 3), "level": r.choice(["error", "info", "warn"]),
               "msg": " ".join(r.choice(WORDS) for _ in range(r.randint(1, 4))), "lat": r.choice([-1.5e-3, 12.25, 7, 1e5])}
        if r.random() < 0.05:
            row["k" * 100] = "timeout=x"                    # a path longer than the device keeps: the row is handed back
        rows.append(row)
    return rows


def cond(t, token=None, field=None):
    c = {"Type": t}
    if field is not None:
        c["Field"] = field
    if token is not None:
        c["Token"] = token
    return {"ExpressionType": "CONDITION", "Condition": c}


QUERIES = [
    (cond("TOKEN", "alice"), None),
    (cond("FIELD_TOKEN", "users", "msg"), None),
    ({"ExpressionType": "AND", "Children": [cond("TOKEN", "timeout"), cond("FIELD_TOKEN", "error", "level")]}, None),
    ({"ExpressionType": "OR", "Children": [cond("TOKEN", "5e"), cond("TOKEN", "miss")]}, None),
    (cond("TOKEN", "alice"), {"ExpressionType": "CONDITION", "Condition": {"Field": "msg", "Pattern": "user=[a-z]+"}}),
    (None, {"ExpressionType": "CONDITION", "Condition": {"Field": "level", "Pattern": "^err"}}),
]


def answer(e, bloom, regex):
    res = e.query(bloom, regex)
    rows = sorted(json.dumps(x, sort_keys=True) for x in res["rows"])
    stats = [(b["FileID"], b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"], b["BytesProcessed"], b["TotalRows"], b["TotalBytes"])
             for b in res["stats"]["BlockStats"]]
    return rows, stats, res["stats"]["Errors"]


def build(ctx, rows, merge, **cfg):
    e = Hst.Engine(ctx, PartitionField="partition", MaxRowGroupRows=100, MaxBufferedRows=300, **cfg)
    for i in range(0, len(rows), 300):
        e.ingest_rows([go_marshal(x) for x in rows[i:i + 300]])
        e.flush()
    if merge:
        e.merge()
    return e


# Every engine gets a context of its own: the library's file-arena cache is per context and keyed by file id, and two engines
# number their files alike.


def test_punctuation_tokenizer_finds_alice():
    row = [b'{"msg":"user=alice"}']
    alice = cond("TOKEN", "alice")
    for device in (False, True):
        for cfg, want in (({"Tokenizer": R.SPECS["punct_lower"]}, ['{"msg": "user=alice"}']), ({}, [])):
            with Context((0,)) as c:
                e = Hst.Engine(c, DeviceIngest=device, DeviceMatch=device, **cfg)
                e.ingest_rows(row)
                e.flush()
                assert [json.dumps(x) for x in e.query(alice)["rows"]] == want, (device, cfg)
                e.close()


@pytest.mark.parametrize("merge", [False, True], ids=["flush", "merge"])
@pytest.mark.parametrize("name", ["punct_lower", "punct_raw", "comma_semi"])
def test_device_switches_do_not_change_answers(name, merge):
    rows = make_rows(3, 900)
    spec = R.SPECS[name]
    got = []
    for device in (False, True):
        with Context((0,)) as c:
            e = build(c, rows, merge, Tokenizer=spec, DeviceIngest=device, DeviceMatch=device, DeviceRegex=device)
            got.append((e.describe(), [answer(e, bloom, regex) for bloom, regex in QUERIES],
                        [e.section_bytes(f, b) for f, fl in enumerate(e.describe()["files"]) for b in range(-1, len(fl["blocks"]))]))
            e.close()
    assert got[0][0] == got[1][0]                                       # counts and filter geometry
    assert got[0][2] == got[1][2]                                       # the filter sections byte for byte
    for (bloom, regex), a, b in zip(QUERIES, got[0][1], got[1][1]):
        assert a == b, (name, bloom, regex)
        want = sorted(json.dumps(x, sort_keys=True) for x in rows if R.row_verdict(go_marshal(x), spec, bloom, regex))
        assert a[0] == want, (name, bloom, regex)
