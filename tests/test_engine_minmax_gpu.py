"""The engine mirror with MinMaxIndexes and Prefilter queries: the three ingest routes (host, DeviceIngest, DeviceIngestStream) describe
identical per-block indexes, equal to the restatement's; merge unions the indexes and keeps blocks with different key sets apart; a
Prefilter drops blocks (and files left without blocks) from the scan and from the stats, per query in bse_query_many; a query
without a prefilter returns what it returned before."""
import json

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import minmax_restatement as MR

pytestmark = pytest.mark.gpu

FIELDS = ["ts", "u"]
PARTS = ["p0", "p1", "p2", "p3"]


def make_rows():
    """400 rows over four partitions with disjoint timestamps: p0 in [0, 100), p1 in [100, 200), p2 in [200, 300); no row of p3 has a
    "ts".  Some rows make the device hand them back: an exponent literal on ts (partition p1), an escaped "t\\u0073" key (p0); some
    timestamps carry a fraction; "u" is a second field with negative values, absent from p2."""
    out = []
    for i in range(400):
        k, n = i % 4, i // 4
        p = PARTS[k]
        ts = k * 100 + n
        if k == 3:
            member = ""
        elif k == 1 and n % 10 == 3:
            member = ',"ts":%d.5e1' % (ts // 10)              # 10.5e1 .. 19.5e1 = 105 .. 195: inside [100, 200)
        elif k == 0 and n % 10 == 7:
            member = ',"t\\u0073":%d' % ts
        elif n % 9 == 4:
            member = ',"ts":%d.25' % ts
        else:
            member = ',"ts":%d' % ts
        u = "" if k == 2 else ',"u":%d' % (-(n * 3) - k)
        out.append(('{"id":%d,"p":"%s","lvl":"%s","msg":"request %d served"%s%s}' % (i, p, "error" if i % 5 == 0 else "info", i, member, u)).encode())
    return out


ROWS = make_rows()
WANT = {p: MR.set_indexes([[r for r in ROWS if json.loads(r)["p"] == p]], FIELDS)[0] for p in PARTS}


def engine(ctx, rows=ROWS, batches=1, **cfg):
    e = Hst.Engine(ctx, PartitionField="p", BloomFalsePositiveRate=1e-6, MaxBufferedRows=100000, MinMaxIndexes=FIELDS, **cfg)
    step = (len(rows) + batches - 1) // batches
    for at in range(0, len(rows), step):
        e.ingest_rows(rows[at: at + step])
    e.flush()
    return e


def block_indexes(e):
    """[(partition id, {field: (min, max)})] of every block, in file / block order"""
    return [(b["PartitionID"], {f: (v["Min"], v["Max"]) for f, v in b.get("MinMaxIndexes", {}).items()}) for f in e.describe()["files"] for b in f["blocks"]]


@pytest.fixture(scope="module")
def engines(ctx):
    made = {"host": engine(ctx), "device": engine(ctx, DeviceIngest=True), "stream": engine(ctx, batches=3, DeviceIngest=True, DeviceIngestStream=True)}
    yield made
    for e in made.values():
        e.close()


def test_the_rows_hold_what_the_cases_need():
    assert WANT["p0"][0] == (0, 99) and WANT["p1"][0] == (100, 199) and WANT["p2"] == [(200, 299), None] and WANT["p3"][0] is None
    assert WANT["p0"][1] == (-297, 0) and WANT["p3"][1] == (-300, -3)
    assert sum(b"e1" in r for r in ROWS) == 10 and sum(b"\\u0073" in r for r in ROWS) == 10


@pytest.mark.parametrize("route", ["host", "device", "stream"])
def test_every_route_describes_the_restatements_indexes(engines, route):
    got = block_indexes(engines[route])
    assert [p for p, _ in got] == PARTS
    for p, idx in got:
        assert idx == {f: WANT[p][i] for i, f in enumerate(FIELDS) if WANT[p][i] is not None}, (route, p)
    blocks = engines[route].describe()["files"][0]["blocks"]
    assert "MinMaxIndexes" in blocks[0] and set(blocks[2]["MinMaxIndexes"]) == {"ts"}
    if route == "stream":
        s = engines[route].describe()["IngestStream"]
        assert s["Batches"] == 3 and s["Flushes"] == 1 and s["HostRows"] >= 20       # the exponent and escaped-key rows came back
    # the filters do not know about the indexes: the routes write the same sections
    assert [engines[route].section_bytes(0, b) for b in range(-1, 4)] == [engines["host"].section_bytes(0, b) for b in range(-1, 4)]


def test_a_block_without_an_index_omits_the_key(ctx):
    e = Hst.Engine(ctx, PartitionField="p", MinMaxIndexes=["nope"], DeviceIngest=True)
    try:
        e.ingest_rows(ROWS[:40])
        e.flush()
        assert all("MinMaxIndexes" not in b for b in e.describe()["files"][0]["blocks"])
    finally:
        e.close()


@pytest.mark.parametrize("cfg", [{}, {"DeviceIngest": True}], ids=["host", "device"])
def test_merge_unions_the_indexes_and_keeps_key_sets_apart(ctx, cfg):
    first = [r for r in ROWS[:200]]
    second = [r.replace(b',"u":', b',"v":') if json.loads(r)["p"] == "p0" else r for r in ROWS[200:]]      # p0's second block has no "u"
    e = Hst.Engine(ctx, PartitionField="p", BloomFalsePositiveRate=1e-6, MaxBufferedRows=100000, MinMaxIndexes=FIELDS, **cfg)
    try:
        for rows in (first, second):
            e.ingest_rows(rows)
            e.flush()
        before = block_indexes(e)
        assert len(before) == 8
        e.merge()
        got = block_indexes(e)
        # p0: key sets {ts, u} and {ts} stay apart; p1, p2, p3 merge to one block each whose index is the union
        assert [p for p, _ in got] == ["p0", "p0", "p1", "p2", "p3"]
        assert got[0] == before[0] and got[1] == before[4]
        for p, idx in got[2:]:
            assert idx == {f: WANT[p][i] for i, f in enumerate(FIELDS) if WANT[p][i] is not None}, p
        # and the rows are all still there
        assert sorted(r["id"] for r in e.query(None)["rows"]) == list(range(400))
    finally:
        e.close()


PREFILTERS = [
    Q.MinMax("ts", "EQ", 150), Q.MinMax("ts", "NE", 150), Q.MinMax("ts", "GT", 200), Q.MinMax("ts", "GTE", 200), Q.MinMax("ts", "LT", 100),
    Q.MinMax("ts", "LTE", 100), Q.MinMax("ts", "IN", 5, 250), Q.MinMax("ts", "NOT_IN", 5, 250), Q.MinMax("ts", "BETWEEN", 50, 120),
    Q.MinMax("ts", "NOT_BETWEEN", 0, 250), Q.MinMax("ts", "BETWEEN", 1000, 2000), Q.MinMax("u", "LT", -298), Q.MinMax("missing", "NOT_IN", 1),
    Q.PrefilterOr(Q.MinMax("ts", "LT", 50), Q.Partition("EQ", "p3")), Q.PrefilterAnd(Q.MinMax("ts", "GTE", 100), Q.Partition("NE", "p2")),
    Q.Partition("IN", "p1", "p3"), Q.Partition("BETWEEN", "p1", "p2"), Q.PrefilterOr(), Q.PrefilterAnd(),
    {"ExpressionType": "CONDITION", "Condition": None},
]


def want_blocks(prefilter):
    return [p for p in PARTS if MR.prefilter_holds(prefilter, p, {f: WANT[p][i] for i, f in enumerate(FIELDS) if WANT[p][i] is not None})]


def check_result(e, res, kept, bloom=None):
    offsets = {b["PartitionID"]: b["BlockOffset"] for b in e.describe()["files"][0]["blocks"]}
    want_rows = [json.loads(r) for p in PARTS if p in kept for r in ROWS if json.loads(r)["p"] == p and (bloom is None or Hst.match_row(bloom, r))]
    assert sorted(r["id"] for r in res["rows"]) == sorted(r["id"] for r in want_rows)
    stats = res["stats"]
    scanned = [b["BlockOffset"] for b in stats["BlockStats"] if not b["BloomFilterSkipped"]]
    assert [b["BlockOffset"] for b in stats["BlockStats"]] == [offsets[p] for p in PARTS if p in kept]   # a block that failed has no entry at all
    if bloom is None:
        assert scanned == [offsets[p] for p in PARTS if p in kept]
    assert stats["FilesConsidered"] == (1 if kept else 0) and stats["FilesBloomSkipped"] == 0


@pytest.mark.parametrize("i", range(len(PREFILTERS)))
def test_a_prefilter_drops_blocks_from_the_scan_and_the_stats(engines, i):
    kept = want_blocks(PREFILTERS[i])
    for route in ("host", "device"):
        check_result(engines[route], engines[route].query(None, prefilter=PREFILTERS[i]), kept)


def test_the_cases_keep_different_block_sets():
    kept = [tuple(want_blocks(p)) for p in PREFILTERS]
    assert kept[0] == ("p1",) and kept[2] == ("p2",) and kept[3] == ("p2",) and kept[10] == () and kept[12] == ()    # a missing index: strictly false
    assert kept[13] == ("p0", "p3") and kept[14] == ("p1",) and kept[17] == () and kept[18] == tuple(PARTS) and len(set(kept)) >= 10


def strip(res):
    """a result without its durations"""
    out = json.loads(json.dumps(res))
    for b in out["stats"]["BlockStats"]:
        b.pop("Duration")
    return out


@pytest.mark.parametrize("cfg", [{}, {"DeviceMatch": True}], ids=["host-match", "device-match"])
def test_query_many_gives_every_query_its_own_prefilter(ctx, cfg):
    e = engine(ctx, **cfg)
    try:
        blooms = [None, Q.FieldToken("lvl", "error"), Q.FieldToken("lvl", "error"), None, Q.Token("served"), None]
        pfs = [PREFILTERS[0], PREFILTERS[3], None, PREFILTERS[10], PREFILTERS[13], None]
        many = e.query_many(blooms, prefilters=pfs)
        for b, pf, res in zip(blooms, pfs, many):
            check_result(e, res, want_blocks(pf) if pf is not None else PARTS, b)
            assert strip(res) == strip(e.query(b, prefilter=pf))
    finally:
        e.close()


def test_a_query_without_a_prefilter_returns_what_it_returned_before(ctx, engines):
    plain = Hst.Engine(ctx, PartitionField="p", BloomFalsePositiveRate=1e-6, MaxBufferedRows=100000)
    try:
        plain.ingest_rows(ROWS)
        plain.flush()
        for bloom in (None, Q.FieldToken("lvl", "error"), Q.And(Q.Field("u"), Q.Token("served"))):
            assert strip(engines["host"].query(bloom)) == strip(plain.query(bloom))
        assert [strip(r) for r in engines["host"].query_many([None, Q.Field("ts")])] == [strip(r) for r in plain.query_many([None, Q.Field("ts")])]
        d_plain, d_mm = plain.describe(), engines["host"].describe()
        for f in d_mm["files"]:
            for b in f["blocks"]:
                b.pop("MinMaxIndexes", None)
        assert d_plain == d_mm
    finally:
        plain.close()
