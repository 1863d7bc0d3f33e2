"""The engine mirror with a "Histogram" member.  Host route: the engine matches as for any query and buckets each matching row with
bsh_hist_row, so a query with the member equals the counts derived from the same query's rows without it (by the restatement,
tests/hist_restatement.py), its "rows" are empty and its stats are the query's without it — through bse_query, through bse_query_many,
and under DeviceMatch with the wide keys, where the rows are matched on the device and bucketed on the host.  Device route
(DeviceMatchHistogram, with DeviceMatch and a wide key): in bse_query_many the histogram queries with an equal spec form wide groups of
their own, ONE bsg_match_rows_wide_hist call per group, the rows it hands back decided on the host; both routes give the same answers."""
import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import hist_restatement as HR

pytestmark = pytest.mark.gpu

PARTS = ["a", "b", "c", "d"]


def make_rows():
    """320 rows over four partitions (one block each); no row of partition d has a timestamp, every sixteenth row (all in partition b)
    writes its timestamp with an exponent, and one row has it under an escaped key"""
    out = []
    for i in range(320):
        p = PARTS[i % 4]
        ts = "" if p == "d" else ',"ts":%s' % ("17000001e%d" % (i % 3) if i % 16 == 1 else str(1700000000 + i) + (".5" if i % 9 == 0 else ""))
        if i == 6:
            ts = ',"t\\u0073":1700000006'
        out.append(('{"id":%d,"partition":"%s","lvl":"%s","msg":"request %d %s"%s}' % (i, p, "error" if i % 5 == 0 else "info", i, "timeout" if i % 7 == 0 else "served", ts)).encode())
    return out


ROWS = make_rows()
SPECS = [{"Field": "ts", "Origin": 1700000000, "Width": 5, "Buckets": 60}, {"Field": "id", "Origin": 10, "Width": 1, "Buckets": 1024},
         {"Field": "ts", "Origin": -(1 << 63), "Width": (1 << 64) - 1, "Buckets": 1}]
QUERIES = [(None, None, None, None), (Q.FieldToken("lvl", "error"), None, None, None), (Q.Token("timeout"), None, None, Q.FieldRange("id", 20, None)),
           (None, Q.FieldRegex("lvl", "^e"), Q.Substring("request 1"), None), (Q.Token("nope"), None, None, None)]


def engine(ctx, **cfg):
    e = Hst.Engine(ctx, PartitionField="partition", BloomFalsePositiveRate=1e-6, MaxBufferedRows=100000, **cfg)
    e.ingest_rows(ROWS)
    e.flush()
    return e


@pytest.fixture(scope="module")
def engines(ctx):
    host = engine(ctx)
    dev = engine(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchWide=True)
    yield host, dev
    host.close()
    dev.close()


def derived(res, spec):
    """{"Counts", "Below", "Above", "Missing"} of a result's rows, by the restatement"""
    B = spec["Buckets"]
    counts = [0] * HR.slots(B)
    for r in res["rows"]:
        counts[HR.slot_of(ROWS[r["id"]], spec["Field"], spec["Origin"], spec["Width"], B)] += 1      # the row as it was ingested: its literals exact
    return {"Counts": counts[:B], "Below": counts[B], "Above": counts[B + 1], "Missing": counts[B + 2]}


def stats_key(res):
    return [(b["FileID"], b["BlockOffset"], b["BloomFilterSkipped"], b["RowsProcessed"], b["TotalRows"]) for b in res["stats"]["BlockStats"]], \
        res["stats"]["FilesConsidered"], res["stats"]["FilesBloomSkipped"]


@pytest.mark.parametrize("spec", range(len(SPECS)))
def test_a_histogram_query_equals_the_counts_of_its_rows(engines, spec):
    host, _ = engines
    for bloom, rx, sx, rg in QUERIES:
        plain = host.query(bloom, rx, sx, rg)
        got = host.query(bloom, rx, sx, rg, histogram=SPECS[spec])
        assert got["rows"] == [] and got["Histogram"] == derived(plain, SPECS[spec])
        assert stats_key(got) == stats_key(plain) and "Histogram" not in plain
        h = got["Histogram"]
        assert sum(h["Counts"]) + h["Below"] + h["Above"] + h["Missing"] == len(plain["rows"])
    every = host.query(histogram=SPECS[0])["Histogram"]
    assert every["Missing"] == 80 and every["Above"] > 0 and every["Counts"][0] > 0 and sum(every["Counts"]) > 100


def test_query_many_and_the_device_matched_rows_give_the_same_counts(engines):
    host, dev = engines
    blooms, rxs, sxs, rgs = zip(*QUERIES)
    specs = [SPECS[0], None, SPECS[1], SPECS[0], SPECS[1]]
    plain = host.query_many(list(blooms), list(rxs), list(sxs), list(rgs))
    for e in (host, dev):
        got = e.query_many(list(blooms), list(rxs), list(sxs), list(rgs), histograms=specs)
        for res, want, spec in zip(got, plain, specs):
            if spec is None:
                assert sorted(r["id"] for r in res["rows"]) == sorted(r["id"] for r in want["rows"]) and "Histogram" not in res
            else:
                assert res["rows"] == [] and res["Histogram"] == derived(want, spec)
            assert stats_key(res)[1:] == stats_key(want)[1:]
    assert sum(dev.match_calls().values()) > 0 and host.match_calls() == {}


def test_a_histogram_spec_beyond_the_limits_is_an_invalid_query(engines):
    host, _ = engines
    for bad in [{"Field": "", "Origin": 0, "Width": 1, "Buckets": 4}, {"Field": "y" * 65, "Origin": 0, "Width": 1, "Buckets": 4},
                {"Field": "ts", "Origin": 0, "Width": 0, "Buckets": 4}, {"Field": "ts", "Origin": 0, "Width": 1, "Buckets": 0},
                {"Field": "ts", "Origin": 0, "Width": 1, "Buckets": 1025}, {"Field": "ts", "Origin": 0.5, "Width": 1, "Buckets": 4},
                {"Field": "ts", "Width": 1, "Buckets": 4}, {"Field": "ts", "Origin": 0, "Width": -1, "Buckets": 4}, "ts"]:
        with pytest.raises(Hst.HostError):
            host.query(histogram=bad)
    assert host.query(histogram={"Field": "y" * 64, "Origin": 0, "Width": 1, "Buckets": 1})["Histogram"]["Missing"] == 320


# ---- the device route ----
MIXING = dict(DeviceMatch=True, DeviceRegex=True, DeviceMatchRangeText=True, DeviceMatchRangeTextWide=True)


@pytest.fixture(scope="module")
def routed(ctx):
    """(host only, the device route under DeviceMatchWide with range and text conditions in one group, the same under DeviceMatchWideRows
    without the mixing keys)"""
    es = [engine(ctx), engine(ctx, DeviceMatchWide=True, DeviceMatchHistogram=True, **MIXING),
          engine(ctx, DeviceMatch=True, DeviceRegex=True, DeviceMatchWideRows=True, DeviceMatchHistogram=True)]
    yield es
    for e in es:
        e.close()


def grown(before, after):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


# token, range, regex and substring queries; every block of partition b holds rows with an exponent on ts, partition c the escaped key
DEVICE_QUERIES = [(None, None, None, None), (Q.FieldToken("lvl", "error"), None, None, None), (Q.Token("timeout"), None, None, Q.FieldRange("id", 20, None)),
                  (None, Q.FieldRegex("lvl", "^e"), None, None), (None, None, Q.Substring("request 1"), None),
                  (Q.Token("served"), Q.FieldRegex("lvl", "^inf"), Q.Substring("quest 2"), Q.FieldRange("ts", 1700000010, 1700000300))]


def test_the_device_route_equals_the_host_route_one_call_per_group(routed):
    host, dev, _ = routed
    blooms, rxs, sxs, rgs = (list(x) for x in zip(*DEVICE_QUERIES))
    plain = host.query_many(blooms, rxs, sxs, rgs)
    for spec in SPECS:
        want = host.query_many(blooms, rxs, sxs, rgs, histograms=[spec] * len(blooms))
        before = dev.match_calls()
        got = dev.query_many(blooms, rxs, sxs, rgs, histograms=[spec] * len(blooms))
        assert grown(before, dev.match_calls()) == {"bsg_match_rows_wide_hist": 1}       # one spec, one group, one call
        for g, w, p in zip(got, want, plain):
            assert g["rows"] == [] and g["Histogram"] == w["Histogram"] == derived(p, spec)
            assert stats_key(g) == stats_key(w)
    # the handed-back rows took part: the exponent rows and the escaped key lie in the blocks every query scans
    every = got[0]["Histogram"]
    assert sum(every["Counts"]) + every["Below"] + every["Above"] + every["Missing"] == 320
    assert host.match_calls() == {}


def test_two_specs_in_one_batch_make_two_groups(routed):
    host, dev, rows_dev = routed
    blooms, rxs, sxs, rgs = (list(x) for x in zip(*DEVICE_QUERIES))
    specs = [SPECS[0], SPECS[1], SPECS[0], SPECS[1], SPECS[0], SPECS[1]]
    plain = host.query_many(blooms, rxs, sxs, rgs)
    before = dev.match_calls()
    got = dev.query_many(blooms, rxs, sxs, rgs, histograms=specs)
    assert grown(before, dev.match_calls()) == {"bsg_match_rows_wide_hist": 2}
    for g, p, spec in zip(got, plain, specs):
        assert g["rows"] == [] and g["Histogram"] == derived(p, spec)
    # a batch of histogram queries and others: the others keep their groups and their rows
    mixed = [SPECS[0], None, SPECS[0], None, None, SPECS[0]]
    before = dev.match_calls()
    got = dev.query_many(blooms, rxs, sxs, rgs, histograms=mixed)
    calls = grown(before, dev.match_calls())
    assert calls.pop("bsg_match_rows_wide_hist") == 1 and sum(calls.values()) >= 1
    for g, p, spec in zip(got, plain, mixed):
        if spec is None:
            assert sorted(r["id"] for r in g["rows"]) == sorted(r["id"] for r in p["rows"]) and "Histogram" not in g
        else:
            assert g["rows"] == [] and g["Histogram"] == derived(p, spec)
    # under DeviceMatchWideRows without the mixing keys: range and text conditions close groups, every group one hist call, the same answers
    before = rows_dev.match_calls()
    got = rows_dev.query_many(blooms, rxs, sxs, rgs, histograms=[SPECS[0]] * len(blooms))
    calls = grown(before, rows_dev.match_calls())
    assert calls.get("bsg_match_rows_wide_hist", 0) >= 2 and not any(k.startswith("bsg_match_rows_wide") and k != "bsg_match_rows_wide_hist" for k in calls)
    for g, p in zip(got, plain):
        assert g["rows"] == [] and g["Histogram"] == derived(p, SPECS[0])
    # bse_query always takes the host route
    before = dev.match_calls()
    one = dev.query(*DEVICE_QUERIES[1], histogram=SPECS[0])
    assert one["Histogram"] == derived(plain[1], SPECS[0]) and "bsg_match_rows_wide_hist" not in grown(before, dev.match_calls())


def test_the_key_without_its_prerequisites_is_an_invalid_config(ctx):
    for cfg in [dict(DeviceMatchHistogram=True), dict(DeviceMatchHistogram=True, DeviceMatch=True), dict(DeviceMatchHistogram=True, DeviceMatchWide=True),
                dict(DeviceMatchHistogram=True, DeviceMatch=True, DeviceMatchLookup=True)]:
        with pytest.raises(Hst.HostError) as e:
            Hst.Engine(ctx, **cfg)
        assert e.value.code == -101
    Hst.Engine(ctx, DeviceMatchHistogram=True, DeviceMatch=True, DeviceMatchWideRows=True).close()
