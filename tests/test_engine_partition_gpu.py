"""The engine mirror with TrustedRows + DevicePartition: every ingest_rows batch goes to a KEYED streaming ingest, the device finds
the rows' partitions and validate_object_row runs only over the rows it hands back.  Yardstick: an engine with DeviceIngestStream
alone (the host parses every row for its partition id) on a context of its own, over the same row stream — what is written and what
queries return must not differ by a byte or a row."""
import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd.gpu import Context
from tests.test_host_tables import KEYS, _random_value, go_marshal

pytestmark = pytest.mark.gpu

FIELDS = ["ts", "v"]


def row_stream(seed, n):
    """about 2 000 rows: five partition values (a number among them: 5 and "5" are one partition), rows without the field, rows with
    escaped values, a partition first seen only in a row the device does not decide, two MinMax fields"""
    rng = np.random.default_rng(seed)
    parts = ['"p0"', '"p1"', '"p2"', '5', '"5"', 'true']
    rows = []
    for i in range(n):
        obj = {KEYS[rng.integers(0, len(KEYS))]: _random_value(rng, 0) for _ in range(rng.integers(1, 4))}
        obj.pop("partition", None)
        obj["msg"] = "Shared WORDS w%d and MiXeD case" % (i % 13)
        obj["level"] = ["info", "error"][i % 2]
        obj["ts"] = 1000 + i
        if i % 5 == 0:
            obj["v"] = i / 4 - 100
        body = go_marshal(obj)
        if i % 17 == 3:
            rows.append(body)                                      # no partition field: the partition ""
        elif i % 2:
            rows.append(b'{"partition":' + parts[(i * 7) % len(parts)].encode() + b"," + body[1:])
        else:
            rows.append(body[:-1] + b',"partition":' + parts[(i * 7) % len(parts)].encode() + b"}")       # the member last
    rows[40] = b'{"partition":"p\\u0031","msg":"escaped value of a known partition","ts":7}'
    rows[41] = b'{"partition":"only\\\\host","msg":"a partition first seen in an undecided row","ts":8}'
    rows[900] = b'{"partition":"only\\\\host","msg":"again","ts":-5,"v":2.5e3}'
    rows[901] = b'{"\\u0070artition":"p2","msg":"escaped key","ts":9}'
    rows[902] = b'{"partition":"p0","deep":' + b'{"a":' * 18 + b'"x"' + b'}' * 18 + b',"ts":3}'
    return rows


def snapshot(e):
    d = e.describe()
    return d, [[e.section_bytes(f, b) for b in range(-1, len(fl["blocks"]))] for f, fl in enumerate(d["files"])]


QUERIES = [(Q.Field("msg"), None), (Q.Token("w7"), Q.Partition("EQ", "p1")), (Q.FieldToken("level", "error"), Q.Partition("IN", "5", "true", "")),
           (Q.Token("partition"), Q.Partition("EQ", "only\\host")), (None, Q.PrefilterAnd(Q.Partition("NE", "p0"), Q.MinMax("ts", "LT", 1500))),
           (Q.Token("escaped"), Q.Partition("GTE", "p1"))]


def test_the_keyed_engine_writes_and_answers_what_the_host_partitioned_engine_does():
    rows = row_stream(11, 2000)
    cuts = [0, 1, 64, 129, 386, 900, 903, 1500, 2000]              # 8 uneven ingest_rows batches
    with Context((0,)) as ca, Context((0,)) as cb:
        cfg = dict(PartitionField="partition", MaxBufferedRows=100000, MaxBufferedBytes=1 << 30, MaxRowGroupRows=100000, DeviceIngest=True,
                   DeviceIngestStream=True, MinMaxIndexes=FIELDS)
        host_parts, keyed = Hst.Engine(ca, **cfg), Hst.Engine(cb, TrustedRows=True, DevicePartition=True, **cfg)
        for lo, hi in zip(cuts, cuts[1:]):
            for e in (host_parts, keyed):
                e.ingest_rows(rows[lo:hi])
            if hi == 900:
                for e in (host_parts, keyed):
                    e.flush()
        for e in (host_parts, keyed):
            e.flush()
        (d0, s0), (d1, s1) = snapshot(host_parts), snapshot(keyed)
        # both files hold the partitions "", 5, only\host, p0, p1, p2, true
        assert len(d0["files"]) == 2 and [len(f["blocks"]) for f in d0["files"]] == [7, 7]
        assert d0["files"] == d1["files"] and s0 == s1             # file and block lists, partition ids, counts, MinMax indexes; sections byte for byte
        assert d1["IngestStream"]["Batches"] == 8 and d1["IngestStream"]["Rows"] == 2000 and d1["IngestStream"]["Flushes"] == 2
        assert d1["IngestStream"]["HostRows"] >= 5 and d0["IngestStream"]["Flushes"] == 2
        d0.pop("IngestStream"), d1.pop("IngestStream")
        assert d0 == d1
        for bloom, pf in QUERIES:
            a, b = host_parts.query(bloom, prefilter=pf), keyed.query(bloom, prefilter=pf)
            assert a["rows"] == b["rows"] and len(a["rows"]) > 0, (bloom, pf)
        for e in (host_parts, keyed):
            e.merge()
        (d0, s0), (d1, s1) = snapshot(host_parts), snapshot(keyed)
        d0.pop("IngestStream"), d1.pop("IngestStream")
        assert d0 == d1 and s0 == s1
        for bloom, pf in QUERIES:
            a, b = host_parts.query(bloom, prefilter=pf), keyed.query(bloom, prefilter=pf)
            assert a["rows"] == b["rows"] and len(a["rows"]) > 0, (bloom, pf)
        for e in (host_parts, keyed):
            e.close()


def test_the_refused_combinations_are_refused_with_a_context(ctx):
    for cfg in (dict(DevicePartition=True, TrustedRows=True, PartitionField="p", DeviceIngest=True),
                dict(DevicePartition=True, PartitionField="p", DeviceIngest=True, DeviceIngestStream=True),
                dict(DevicePartition=True, TrustedRows=True, DeviceIngest=True, DeviceIngestStream=True)):
        with pytest.raises(Hst.HostError) as err:
            Hst.Engine(ctx, **cfg)
        assert err.value.code == -101
    Hst.Engine(ctx, DevicePartition=True, TrustedRows=True, PartitionField="p", DeviceIngest=True, DeviceIngestStream=True).close()
    # TrustedRows alone: nothing is asked of a row at ingest time, and nothing else changes
    e = Hst.Engine(ctx, TrustedRows=True, DeviceIngest=True)
    e.ingest_rows([b'{"a":"x y"}', b'{"a":"z"}'])
    e.flush()
    assert len(e.query(Q.Token("z"))["rows"]) == 1
    e.close()
