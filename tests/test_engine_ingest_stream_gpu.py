"""The engine mirror with DeviceIngestStream: every ingest_rows batch goes to an open streaming ingest when it arrives
(bsg_ingest_open / bsg_ingest_add_sets / bsg_ingest_append_rows) and flush only finishes, sizes and builds.  Yardstick: an
engine with DeviceIngest alone (the one-shot bsg_ingest_rows_tok at flush time) on a context of its own, over the same row
stream — what is written and what queries return must not differ by a byte or a row."""
import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd.gpu import Context
from tests.test_host_tables import KEYS, _random_value, go_marshal

pytestmark = pytest.mark.gpu


def row_stream(seed, n):
    """3 partitions, p2 met first (sets are numbered by first arrival, blocks by partition id); escapes and UTF-8
    in about half the rows, so some are handed back to the host walker"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        obj = {KEYS[rng.integers(0, len(KEYS))]: _random_value(rng, 0) for _ in range(rng.integers(1, 5))}
        obj["partition"] = "p%d" % ((i + 2) % 3 if i >= 5 else 2)
        obj["msg"] = "Shared WORDS w%d and MiXeD case" % (i % 13)
        obj["level"] = ["info", "error"][i % 2]
        rows.append(go_marshal(obj))
    rows[7] = b'{"partition":"p0","deep":' + b'{"a":' * 18 + b'"x"' + b'}' * 18 + b'}'      # beyond the device walker: finished at once
    return rows


def snapshot(e):
    d = e.describe()
    return d, [[e.section_bytes(f, b) for b in range(-1, len(fl["blocks"]))] for f, fl in enumerate(d["files"])]


def test_streamed_flush_writes_and_answers_what_the_one_shot_flush_does():
    rows = row_stream(3, 350)
    cuts = [0, 1, 6, 70, 134, 199, 200, 350]                              # 7 ingest_rows batches
    with Context((0,)) as ca, Context((0,)) as cb:
        cfg = dict(PartitionField="partition", MaxBufferedRows=100000, MaxBufferedBytes=1 << 30, DeviceIngest=True)
        one_shot, stream = Hst.Engine(ca, **cfg), Hst.Engine(cb, DeviceIngestStream=True, **cfg)
        for e in (one_shot, stream):
            for lo, hi in zip(cuts, cuts[1:]):
                e.ingest_rows(rows[lo:hi])
            e.flush()
        (d0, s0), (d1, s1) = snapshot(one_shot), snapshot(stream)
        assert len(d0["files"]) == 1 and len(d0["files"][0]["blocks"]) == 3
        assert d0["files"] == d1["files"] and s0 == s1                    # block and file sections, per-block counts
        # ... and the streamed path did the work: all 7 batches went to the stream when they arrived, the deep row was finished by
        # the host walker right then, the flush was built from the stream; the other engine streamed nothing
        assert d1["IngestStream"] == {"Batches": 7, "Rows": 350, "HostRows": d1["IngestStream"]["HostRows"], "Flushes": 1}
        assert d1["IngestStream"]["HostRows"] >= 1
        assert d0["IngestStream"] == {"Batches": 0, "Rows": 0, "HostRows": 0, "Flushes": 0}
        queries = [Q.Field("msg"), Q.Token("w7"), Q.And(Q.FieldToken("level", "error"), Q.Token("shared"))]
        for q in queries:
            a, b = one_shot.query(q), stream.query(q)
            assert a["rows"] == b["rows"] and len(a["rows"]) > 0, q
        # a second flush after more batches: the stream was reopened (new partition p3 first this time)
        more = row_stream(4, 120)
        more[0] = go_marshal({"partition": "p3", "msg": "late partition"})
        for e in (one_shot, stream):
            e.ingest_rows(more[:50])
            e.ingest_rows(more[50:])
            e.flush()
        (d0, s0), (d1, s1) = snapshot(one_shot), snapshot(stream)
        assert len(d0["files"]) == 2 and len(d0["files"][1]["blocks"]) == 4 and d0["files"] == d1["files"] and s0 == s1
        assert (d1["IngestStream"]["Batches"], d1["IngestStream"]["Rows"], d1["IngestStream"]["Flushes"]) == (9, 470, 2)
        assert d0["IngestStream"]["Batches"] == 0 and d0["IngestStream"]["Flushes"] == 0
        for q in queries + [Q.Token("late")]:
            a, b = one_shot.query(q), stream.query(q)
            assert a["rows"] == b["rows"] and len(a["rows"]) > 0, q
        for e in (one_shot, stream):
            e.close()


def test_stream_without_device_ingest_is_refused_at_open(ctx):
    with pytest.raises(Hst.HostError) as err:
        Hst.Engine(ctx, DeviceIngestStream=True)
    assert err.value.code == -101                                         # ErrInvalidConfig
    with pytest.raises(Hst.HostError):
        Hst.Engine(ctx, DeviceIngestStream=True, DeviceIngest=False)
    Hst.Engine(ctx, DeviceIngestStream=False).close()

