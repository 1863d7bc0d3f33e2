"""bse_query_many / BloomSearchEngine::query_many: element i of the batch's result equals what the existing query() returns for
query i alone - rows in the same order, every BlockStats field but the duration, Errors, FilesConsidered, FilesBloomSkipped -
with DeviceMatch on and off, under the default and a configured tokenizer, for batches over 64 queries, with a regex query in
the middle, and for the empty batch."""
import random

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import tokenizer_restatement as TR
from tests.test_host_tables import go_marshal

pytestmark = pytest.mark.gpu

WORDS = ["timeout", "retry", "cache", "miss", "ok", "disk", "full", "user=alice", "bob,carol", "Login", "failed"]
LEVELS = ["error", "info", "warn", "debug"]
SERVICES = ["payments", "auth", "search", "pay-gw"]


def make_rows(seed, n):
    r = random.Random(seed)
    rows = []
    for i in range(n):
        p = i % 7
        # levels and services depend on the partition, so that queries survive on different blocks of one file
        row = {"id": i, "partition": "p%d" % p, "level": LEVELS[(p + r.randint(0, 1)) % 4], "service": SERVICES[(p // 2 + r.randint(0, 1)) % 4],
               "message": " ".join(r.choice(WORDS) for _ in range(r.randint(1, 5))), "user": {"name": r.choice(["john", "Jane", "bob"]), "id": p}}
        if r.random() < 0.04:
            row["k" * 100] = "timeout"                      # a path longer than the device keeps: the row is handed back
        if p == 6 and r.random() < 0.3:
            row["only6"] = "needle-%d" % (i % 5)
        rows.append(row)
    return rows


def build(ctx, **cfg):
    e = Hst.Engine(ctx, PartitionField="partition", MaxRowGroupRows=100000, MaxBufferedRows=100000, BloomFalsePositiveRate=1e-4, **cfg)
    rows = make_rows(5, 2100)
    for i in range(0, len(rows), 700):
        e.ingest_rows([go_marshal(x) for x in rows[i:i + 700]])
        e.flush()
    return e


def comparable(res):
    stats = [(b["FileID"], b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"], b["BytesProcessed"], b["TotalRows"], b["TotalBytes"])
             for b in res["stats"]["BlockStats"]]
    return res["rows"], stats, res["stats"]["Errors"], res["stats"]["FilesConsidered"], res["stats"]["FilesBloomSkipped"]


def queries(n, seed=3):
    r = random.Random(seed)
    fixed = [None, Q.FieldToken("only6", "needle-2"), Q.Token("never-there"), Q.Field("user.name"), Q.And(), Q.Or(),
             Q.And(Q.FieldToken("level", "error"), Q.FieldToken("service", "payments")), Q.FieldToken("partition", "p3"),
             Q.Or(Q.FieldToken("partition", "p1"), Q.FieldToken("user.id", "5")), Q.Token("timeout"), Q.Field("k" * 100),
             Q.And(Q.Token("timeout"), Q.Field("k" * 100)), {"ExpressionType": "XOR", "Children": []}]
    out = list(fixed)
    while len(out) < n:
        kind = r.randint(0, 3)
        if kind == 0:
            out.append(Q.And(Q.FieldToken("level", r.choice(LEVELS)), Q.FieldToken("service", r.choice(SERVICES)), Q.Token(r.choice(WORDS).lower())))
        elif kind == 1:
            out.append(Q.Or(Q.FieldToken("partition", "p%d" % r.randint(0, 8)), Q.FieldToken("only6", "needle-%d" % r.randint(0, 6))))
        elif kind == 2:
            out.append(Q.And(Q.FieldToken("user.id", str(r.randint(0, 7))), Q.Or(Q.Token(r.choice(WORDS).lower()), Q.FieldToken("user.name", "jane"))))
        else:
            out.append(Q.FieldToken("message", r.choice(["alice", "bob", "carol", "login", "user=alice", "bob,carol"])))
    return out[:n]


def check(e, exprs, regexes=None):
    got = e.query_many(exprs, regexes)
    assert len(got) == len(exprs)
    n_rows = pruned = partial = 0
    for i, x in enumerate(exprs):
        want = comparable(e.query(x, None if regexes is None else regexes[i]))
        assert comparable(got[i]) == want, (i, x)
        n_rows += len(want[0])
        skipped = [s[2] for s in want[1]]
        pruned += any(skipped)
        partial += any(skipped) and not all(skipped)
    return n_rows, pruned, partial


@pytest.mark.parametrize("device_match", [False, True])
def test_batch_equals_single_queries(ctx, device_match):
    e = build(ctx, DeviceMatch=device_match)
    try:
        assert max(len(f["blocks"]) for f in e.describe()["files"]) >= 7                      # files hold several blocks
        n_rows, pruned, partial = check(e, queries(40))
        assert n_rows > 100 and pruned >= 5 and partial >= 3                               # queries survive on different blocks
        assert e.query_many([]) == []
        assert check(e, [Q.FieldToken("only6", "needle-2")])[0] > 0                           # a batch of one
        assert check(e, [None, None])[0] == 4200
    finally:
        e.close()


@pytest.mark.parametrize("device_match", [False, True])
def test_more_than_64_queries_and_more_than_64_conditions(ctx, device_match):
    e = build(ctx, DeviceMatch=device_match)
    try:
        n_rows, pruned, _ = check(e, queries(150, seed=8))
        assert n_rows > 100 and pruned > 10
        wide = [Q.Or(*[Q.FieldToken("user.id", str(k)) for k in range(70)]),                  # 70 conditions in one query: the host matcher's
                Q.And(*[Q.Or(Q.Token("t%d" % i), Q.Field("id")) for i in range(40)])] + queries(20)
        assert check(e, wide)[0] >= 2100
    finally:
        e.close()


@pytest.mark.parametrize("device", [False, True])
def test_regex_query_in_the_middle(ctx, device):
    e = build(ctx, DeviceMatch=device, DeviceRegex=device)
    try:
        exprs = queries(9) + [Q.FieldToken("level", "error"), None] + queries(30)[20:]
        regexes = [None] * 9 + [Q.FieldRegex("message", "timeout|cache"), Q.FieldRegex("service", "^pay")] + [None] * 10
        n_rows, _, _ = check(e, exprs, regexes)
        assert n_rows > 100
        got = e.query_many(exprs, regexes)
        assert 0 < len(got[9]["rows"]) < 2100 and all("pay" in r["service"] for r in got[10]["rows"]) and got[10]["rows"]
    finally:
        e.close()


@pytest.mark.parametrize("device_match", [False, True])
def test_configured_tokenizer(ctx, device_match):
    e = build(ctx, DeviceMatch=device_match, DeviceIngest=device_match, Tokenizer=TR.SPECS["punct_lower"])
    try:
        exprs = queries(30) + [Q.Token("alice"), Q.FieldToken("message", "carol"), Q.Token("gw"), Q.FieldToken("service", "pay")]
        n_rows, pruned, _ = check(e, exprs)
        assert n_rows > 100 and pruned >= 5
        got = e.query_many(exprs)
        assert got[30]["rows"] and all("alice" in r["message"] for r in got[30]["rows"])       # "user=alice" splits under this tokenizer only
        assert got[32]["rows"] and all(r["service"] == "pay-gw" for r in got[32]["rows"])
    finally:
        e.close()


def test_unreadable_block_filters_are_reported_per_query(ctx):
    e = build(ctx, DeviceMatch=True)
    try:
        e.corrupt_section_byte(1, 2, 40)
        exprs = queries(12)
        check(e, exprs)
        got = e.query_many(exprs)
        assert got[0]["stats"]["Errors"] == [] and any(g["stats"]["Errors"] for g in got[1:])  # the nil query reads no filters
    finally:
        e.close()
