"""The engine mirror with a "Tokenizer" that carries an n-gram width ("Ngram": 3): the substring "imeou" is found inside
"error:timeout" as the AND of its trigrams, which no word tokenizer can; and with the device-routing keys on and off the rows,
BlockStats, the filters bse_describe reports and the filter sections are identical, through flushes and a merge, and equal the
restatement's verdicts (tests/ngram_restatement.py)."""
import json

import pytest

from bloomsearch_amd import host as Hst
from bloomsearch_amd.gpu import Context
from tests import ngram_restatement as G
from tests.test_engine_tokenizer_gpu import answer, build, cond, make_rows
from tests.test_host_tables import go_marshal

pytestmark = pytest.mark.gpu

AND = lambda *kids: {"ExpressionType": "AND", "Children": list(kids)}
QUERIES = [
    (AND(cond("TOKEN", "ime"), cond("TOKEN", "meo"), cond("TOKEN", "eou")), None),                  # the substring imeou
    (AND(cond("FIELD_TOKEN", "=al", "msg"), cond("FIELD_TOKEN", "ali", "msg")), None),              # =ali under msg
    (cond("TOKEN", "ok"), None),                                                                    # a short word, whole
    (cond("TOKEN", "timeout"), None),                                                               # a whole long word is no token
    ({"ExpressionType": "OR", "Children": [cond("TOKEN", "5e-"), cond("FIELD_TOKEN", "rro", "level")]}, None),
    (cond("TOKEN", "che"), {"ExpressionType": "CONDITION", "Condition": {"Field": "msg", "Pattern": "user=[a-z]+"}}),
]
DEVICE_KEYS = [dict(DeviceIngest=True, DeviceMatch=True, DeviceRegex=True),
               dict(DeviceIngest=True, DeviceIngestStream=True, DeviceMatch=True, DeviceRegex=True, DeviceMatchWide=True),
               dict(DeviceIngest=True, DeviceMatch=True, DeviceRegex=True, DeviceMatchLookup=True, DeviceMatchLookupRegex=True)]


def test_trigrams_find_a_substring():
    rows = [b'{"msg":"error:timeout"}', b'{"msg":"time out"}']
    needle = QUERIES[0][0]
    for device in (False, True):
        for cfg, want in (({"Tokenizer": G.SPECS["tri_default"]}, ['{"msg": "error:timeout"}']), ({}, [])):
            with Context((0,)) as c:
                e = Hst.Engine(c, DeviceIngest=device, DeviceMatch=device, **cfg)
                e.ingest_rows(rows)
                e.flush()
                assert [json.dumps(x) for x in e.query(needle)["rows"]] == want, (device, cfg)
                e.close()


@pytest.mark.parametrize("merge", [False, True], ids=["flush", "merge"])
def test_device_switches_do_not_change_answers(merge):
    rows = make_rows(3, 900)
    spec = G.SPECS["tri_default"]
    got = []
    for keys in [dict()] + DEVICE_KEYS:
        with Context((0,)) as c:
            e = build(c, rows, merge, Tokenizer=spec, **keys)
            got.append((e.describe(), [answer(e, bloom, regex) for bloom, regex in QUERIES],
                        [e.section_bytes(f, b) for f, fl in enumerate(e.describe()["files"]) for b in range(-1, len(fl["blocks"]))]))
            # the batch in one pass (bse_query_many: the many / wide / lookup calls under their keys) answers like the single queries
            many = e.query_many([q for q, _ in QUERIES], [x for _, x in QUERIES])
            assert [sorted(json.dumps(x, sort_keys=True) for x in m["rows"]) for m in many] == [a[0] for a in got[-1][1]], keys
            e.close()
    for other in got[1:]:
        assert got[0][0]["files"] == other[0]["files"]                   # counts and filter geometry
        assert got[0][2] == other[2]                                     # the filter sections byte for byte
        for (bloom, regex), a, b in zip(QUERIES, got[0][1], other[1]):
            assert a == b, (bloom, regex)
    for (bloom, regex), a in zip(QUERIES, got[0][1]):
        want = sorted(json.dumps(x, sort_keys=True) for x in rows if G.row_verdict(go_marshal(x), spec, bloom, regex))
        assert a[0] == want, (bloom, regex)
    assert got[0][1][0][0] and got[0][1][2][0] and not got[0][1][3][0]   # imeou and ok are found; "timeout" as one token is not
