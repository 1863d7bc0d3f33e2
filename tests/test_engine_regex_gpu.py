"""The engine mirror with DeviceMatch + DeviceRegex (regex queries matched bloom AND regex by one bsg_match_rows_regex call, the
rows the device hands back by the host matcher on the same DFAs) returns the same rows and BlockStats as with both switches off
(std::regex on the host), for the reference's regex queries and random patterns where RE2 and std::regex agree."""
import json
import random

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests.test_host_tables import go_marshal

pytestmark = pytest.mark.gpu

WORDS = ["timeout", "retry", "cache", "miss", "payment", "error", "info", "warn", "db", "shard", "ok", "x", "Timeout", "ERROR"]


def make_rows(seed, n):
    r = random.Random(seed)
    rows = []
    for i in range(n):
        row = {"id": i, "partition": "p%d" % (i % 3), "level": r.choice(["error", "info", "warn", "debug"]),
               "service": r.choice(["payments", "auth", "search", "pay-gw"]),
               "message": " ".join(r.choice(WORDS) for _ in range(r.randint(1, 6))),
               "user": {"name": r.choice(["john", "Jane", "bob"]), "id": r.randint(0, 9), "active": r.random() < 0.5}}
        if r.random() < 0.3:
            row["tags"] = [r.choice(WORDS) for _ in range(r.randint(0, 3))]
        if r.random() < 0.05:
            row["k" * 100] = "timeout"                      # a path longer than the device keeps: the row is handed back
        rows.append(row)
    return rows


def random_pattern(r):
    atoms = [r.choice(WORDS), "[0-9]", "[a-z]+", ".", "o+", "e?r", "(" + r.choice(WORDS) + "|" + r.choice(WORDS) + ")", "[^ ]*"]
    p = "".join(r.choice(atoms) for _ in range(r.randint(1, 3)))
    if r.random() < 0.3:
        p = "^" + p
    if r.random() < 0.3:
        p = p + "$"
    return p


def answer(e, bloom, regex):
    res = e.query(bloom, regex)
    rows = sorted(json.dumps(x, sort_keys=True) for x in res["rows"])
    stats = [(b["FileID"], b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"], b["BytesProcessed"], b["TotalRows"], b["TotalBytes"])
             for b in res["stats"]["BlockStats"]]
    return rows, stats, res["stats"]["Errors"], res["stats"]["FilesConsidered"], res["stats"]["FilesBloomSkipped"]


@pytest.fixture
def engines(ctx):
    rows = make_rows(1, 900)
    out = []
    for cfg in ({"DeviceMatch": False, "DeviceRegex": False}, {"DeviceMatch": True, "DeviceRegex": True}):
        e = Hst.Engine(ctx, PartitionField="partition", MaxRowGroupRows=100, MaxBufferedRows=300, **cfg)
        for i in range(0, len(rows), 300):
            e.ingest_rows([go_marshal(x) for x in rows[i:i + 300]])
            e.flush()
        out.append(e)
    yield out
    for e in out:
        e.close()


def test_reference_regex_queries_agree(engines):
    off, on = engines
    queries = [
        (None, Q.RegexOr(Q.RegexAnd(Q.FieldRegex("message", "timeout|retry"), Q.FieldRegex("level", "^err")), Q.FieldRegex("service", "^pay"))),
        (Q.FieldToken("level", "error"), Q.FieldRegex("message", "timeout|cache")),          # the QueryRegex bench shape
        (None, Q.RegexAnd(Q.FieldRegex("user.name", "(?i)^jo"), Q.RegexOr(Q.FieldRegex("user.active", "^true$"), Q.FieldRegex("user.id", "^2$")))),
        (Q.Field("user"), Q.FieldRegex("user", "^[0-9]+$")),
        (Q.Token("ok"), Q.FieldRegex("tags", "miss")),
        (None, Q.FieldRegex("message", "\\Azzz-never-matches\\z")),
        (None, Q.FieldRegex("k" * 100, "time")),
        (None, Q.RegexOr()),
        (None, Q.RegexAnd()),
        (None, Q.FieldRegex("", ".*")),
        (None, Q.FieldRegex("no.such.path", ".*")),
    ]
    nonempty = 0
    for bloom, rx in queries:
        if rx is not None and "\\z" in json.dumps(rx):
            # \A / \z are RE2 text anchors that std::regex does not share: only the device path is compared, with what RE2 answers
            assert answer(on, bloom, rx)[0] == []
            continue
        a = answer(off, bloom, rx)
        assert answer(on, bloom, rx) == a, (bloom, rx)
        nonempty += bool(a[0])
    assert nonempty >= 6


def test_random_subset_patterns_agree(engines):
    off, on = engines
    r = random.Random(5)
    fields = ["message", "level", "service", "user", "user.name", "tags"]
    for _ in range(60):
        rx = Q.FieldRegex(r.choice(fields), random_pattern(r))
        if r.random() < 0.4:
            rx = (Q.RegexAnd if r.random() < 0.5 else Q.RegexOr)(rx, Q.FieldRegex(r.choice(fields), random_pattern(r)))
        bloom = r.choice([None, Q.Token("timeout"), Q.Field("tags"), Q.FieldToken("level", "info")])
        assert answer(on, bloom, rx) == answer(off, bloom, rx), (bloom, rx)
