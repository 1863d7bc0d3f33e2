"""What partitioning on the device buys and costs (k_partition_rows / k_partition_assign, csrc/partition.hip.h), on synth log rows with a
partition member added: 16 and 1 024 values, the member first and last in the row, batches of 50 000 rows.

  (a)  HEADLINE: wall time of the engine's bse_ingest_rows over the whole stream (no flush inside the timed region) with
       DeviceIngestStream + TrustedRows + DevicePartition in this library, against DeviceIngestStream alone with the same PartitionField
       in the library given by --parent-lib (the parent commit's; without the option: this library with the two keys off, which runs
       the parent's code path).  The difference is the host parse the keys remove (validate_object_row over every row) less what the
       partition pass adds.  Bar: lower by more than the two runs' combined spread.
  (b)  DEVICE COST: bsg_last_partition_ms summed over the stream's bsg_ingest_append_rows_keyed calls, against the MinMax scanner with
       ONE field (the partition member) over the same rows - the same scan without the lookup and without the early stop: once as
       bsg_last_minmax_ms of one bsg_ingest_rows_minmax call over all rows, and once summed over the same batches through
       bsg_ingest_open_minmax / bsg_ingest_append_rows (a batch of 50 000 rows does not fill the device: a dispatch then costs the
       scan of its longest rows however few they are, so twenty batches cost more than one call).  Bar, against each: not above it by
       more than that measurement's spread.
  (c)  WALK: ms_walk (bsg_ingest_stats) of the keyed stream against a stream fed through bsg_ingest_append_rows with the same sets
       (--parent-lib: in the parent's library).  Bar: equal within the spread; the walkers are untouched.

One untimed warm-up round, then R timed rounds with the legs alternating; every figure is the median with its spread (min .. max).
Every bar is written down as MET or NOT MET with the figures.  The keys stay opt-in and no routing rule is derived from this file.

    python tools/ingest_partition_lab.py [n_rows] [rounds] [--parent-lib PATH/libbloomgpu.so] [--out profiles/ingest_partition_lab.txt]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import _lib, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
args = [a for a in args if a not in opts.values()]
n_rows = int(args[0]) if args else 1_000_000
rounds = int(args[1]) if len(args) > 1 else 5
BATCH = 50_000
FIELD = "tenant"


class Lib:
    """the few calls this tool makes, bound on a library of its own (this commit's, or the parent commit's)"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
        L.bsg_open.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
        L.bsg_close.argtypes = [vp]
        L.bsg_last_error.argtypes = [vp]
        L.bsg_last_error.restype = C.c_char_p
        L.bsg_ingest_rows_minmax.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, C.POINTER(u64), vp, vp, u32]
        L.bsg_last_minmax_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.bsg_ingest_open.argtypes = [vp, u32, vp, u32, vp, u32, vp, C.POINTER(u64)]
        L.bsg_ingest_open_minmax.argtypes = L.bsg_ingest_open.argtypes + [vp, vp, u32]
        L.bsg_ingest_add_sets.argtypes = [vp, u64, u32, vp, vp, C.POINTER(u32)]
        L.bsg_ingest_append_rows.argtypes = [vp, u64, vp, vp, u32, vp, vp, u32, C.POINTER(u32)]
        L.bsg_ingest_stats_read.argtypes = [vp, u64, C.POINTER(_lib.IngestStats)]
        L.bsg_ingest_free.argtypes = [vp, u64]
        L.bse_open.argtypes = [C.c_char_p, u64, vp, C.POINTER(vp)]
        L.bse_close.argtypes = [vp]
        L.bse_close.restype = None
        L.bse_last_error.argtypes = [vp]
        L.bse_last_error.restype = C.c_char_p
        L.bse_ingest_rows.argtypes = [vp, vp, u64]
        self.keyed = hasattr(L, "bsg_ingest_open_keyed")
        if self.keyed:
            L.bsg_ingest_open_keyed.argtypes = [vp, u32, u32, u32, vp, C.POINTER(u64), C.c_char_p, u32, vp, vp, u32]
            L.bsg_ingest_append_rows_keyed.argtypes = [vp, u64, vp, vp, u32, vp, C.POINTER(u32), vp, u32, C.POINTER(u32)]
            L.bsg_last_partition_ms.argtypes = [vp, C.POINTER(C.c_float)]
        self.h = vp()
        ids = (i32 * 1)(0)
        self.check(L.bsg_open(ids, 1, C.byref(self.h)))

    def check(self, rc):
        if rc:
            raise RuntimeError("libbloomgpu error %d: %s" % (rc, self.L.bsg_last_error(self.h).decode()))

    def engine_ingest(self, batches, **keys):
        """wall seconds of bse_ingest_rows over the batches (NDJSON blobs); nothing is flushed inside"""
        big = 1 << 40
        cfg = json.dumps(dict(PartitionField=FIELD, DeviceIngest=True, DeviceIngestStream=True, MaxBufferedRows=big, MaxBufferedBytes=big,
                              MaxRowGroupRows=big, MaxRowGroupBytes=big, **keys)).encode()
        e = C.c_void_p()
        rc = self.L.bse_open(cfg, len(cfg), self.h, C.byref(e))
        if rc:
            raise RuntimeError("bse_open: %d" % rc)
        t = 0.0
        try:
            for nd in batches:
                t0 = time.perf_counter()
                rc = self.L.bse_ingest_rows(e, nd.ctypes.data, len(nd))
                t += time.perf_counter() - t0
                if rc:
                    raise RuntimeError("bse_ingest_rows: %d %s" % (rc, self.L.bse_last_error(e).decode()))
        finally:
            self.L.bse_close(e)
        return t

    def keyed_stream(self, parts):
        """-> (sum of bsg_last_partition_ms, ms_walk, the batches' sets, rows handed back)"""
        ing, ms, n_fb, n_new = C.c_uint64(), C.c_float(), C.c_uint32(), C.c_uint32()
        self.check(self.L.bsg_ingest_open_keyed(self.h, 1, 0, _lib.INGEST_TRUSTED_JSON, None, C.byref(ing), FIELD.encode(), len(FIELD), None, None, 0))
        total, sets, handed = 0.0, [], 0
        try:
            for blob, off in parts:
                n = len(off) - 1
                sor, fb = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
                self.check(self.L.bsg_ingest_append_rows_keyed(self.h, ing, blob.ctypes.data, off.ctypes.data, n, sor.ctypes.data, C.byref(n_new),
                                                               fb.ctypes.data, n, C.byref(n_fb)))
                self.check(self.L.bsg_last_partition_ms(self.h, C.byref(ms)))
                total += float(ms.value)
                handed += int(n_fb.value)
                sets.append(sor)
            st = _lib.IngestStats()
            self.check(self.L.bsg_ingest_stats_read(self.h, ing, C.byref(st)))
            return total, float(st.ms_walk), sets, handed
        finally:
            self.L.bsg_ingest_free(self.h, ing)

    def plain_stream(self, parts, sets):
        """the same batches through bsg_ingest_append_rows with the given sets, the partition member as the one MinMax field
        -> (ms_walk, sum of bsg_last_minmax_ms)"""
        ing, n_fb, first, ms = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_float()
        name = np.frombuffer(FIELD.encode(), dtype=np.uint8).copy()
        fo = np.array([0, len(name)], dtype=np.uint32)
        self.check(self.L.bsg_ingest_open_minmax(self.h, 0, None, 1, None, _lib.INGEST_TRUSTED_JSON, None, C.byref(ing), name.ctypes.data, fo.ctypes.data, 1))
        have, mm = 0, 0.0
        try:
            for (blob, off), sor in zip(parts, sets):
                n = len(off) - 1
                top = int(sor.max()) + 1
                if top > have:
                    parent = np.zeros(top - have, dtype=np.uint32)
                    self.check(self.L.bsg_ingest_add_sets(self.h, ing, top - have, parent.ctypes.data, None, C.byref(first)))
                    have = top
                fb = np.zeros(n, dtype=np.uint32)
                self.check(self.L.bsg_ingest_append_rows(self.h, ing, blob.ctypes.data, off.ctypes.data, n, sor.ctypes.data, fb.ctypes.data, n, C.byref(n_fb)))
                self.check(self.L.bsg_last_minmax_ms(self.h, C.byref(ms)))
                mm += float(ms.value)
            st = _lib.IngestStats()
            self.check(self.L.bsg_ingest_stats_read(self.h, ing, C.byref(st)))
            return float(st.ms_walk), mm
        finally:
            self.L.bsg_ingest_free(self.h, ing)

    def minmax_scan(self, blob, off):
        """bsg_last_minmax_ms of one bsg_ingest_rows_minmax call over all rows as one set, one field: the partition member"""
        ing, ms = C.c_uint64(), C.c_float()
        first = np.array([0, len(off) - 1], dtype=np.uint32)
        name = np.frombuffer(FIELD.encode(), dtype=np.uint8).copy()
        fo = np.array([0, len(name)], dtype=np.uint32)
        self.check(self.L.bsg_ingest_rows_minmax(self.h, blob.ctypes.data, off.ctypes.data, len(off) - 1, first.ctypes.data, 1, None, 0, None,
                                                 _lib.INGEST_TRUSTED_JSON, None, C.byref(ing), name.ctypes.data, fo.ctypes.data, 1))
        self.check(self.L.bsg_last_minmax_ms(self.h, C.byref(ms)))
        self.L.bsg_ingest_free(self.h, ing)
        return float(ms.value)


def med(xs):
    return "%8.2f  (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def spread(xs):
    return max(xs) - min(xs)


def make_rows(n_values, member_first):
    base = synth.rows_json(0, n_rows)
    if member_first:
        return [b'{"%s":"t%04d",' % (FIELD.encode(), (i * 7919) % n_values) + r[1:] for i, r in enumerate(base)]
    return [r[:-1] + b',"%s":"t%04d"}' % (FIELD.encode(), (i * 7919) % n_values) for i, r in enumerate(base)]


def main():
    here = Lib(os.path.join(ROOT, "bloomsearch_amd", "csrc", "libbloomgpu.so"))
    parent = Lib(opts["--parent-lib"]) if "--parent-lib" in opts else here
    base_name = "the parent commit's library" if parent is not here else "this library with the two keys off (the parent's code path)"
    lines = ["ingest_partition_lab: %d synth rows, batches of %d, %d rounds after one warm-up; ms, median (min .. max)" % (n_rows, BATCH, rounds),
             "baseline: " + base_name, ""]
    for n_values in (16, 1024):
        for member_first in (True, False):
            rows = make_rows(n_values, member_first)
            nd = [np.frombuffer(b"\n".join(rows[i: i + BATCH]) + b"\n", dtype=np.uint8) for i in range(0, n_rows, BATCH)]
            parts = []
            for i in range(0, n_rows, BATCH):
                chunk = rows[i: i + BATCH]
                off = np.zeros(len(chunk) + 1, dtype=np.uint64)
                off[1:] = np.cumsum([len(r) for r in chunk], dtype=np.uint64)
                parts.append((np.frombuffer(b"".join(chunk), dtype=np.uint8), off))
            all_off = np.zeros(n_rows + 1, dtype=np.uint64)
            all_off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
            all_blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
            n_bytes = int(all_off[-1])
            del rows
            t_keyed, t_base, p_ms, w_keyed, w_plain, m_ms, mb_ms = [], [], [], [], [], [], []
            handed = 0
            for r in range(rounds + 1):
                a = here.engine_ingest(nd, TrustedRows=True, DevicePartition=True) * 1e3
                b = parent.engine_ingest(nd) * 1e3
                p, w, sets, handed = here.keyed_stream(parts)
                wp, mb = parent.plain_stream(parts, sets)
                m = parent.minmax_scan(all_blob, all_off)
                if r:
                    t_keyed.append(a), t_base.append(b), p_ms.append(p), w_keyed.append(w), w_plain.append(wp), m_ms.append(m), mb_ms.append(mb)
            removed = statistics.median(t_base) - statistics.median(t_keyed)
            lines += ["%d values, the member %s (%.0f MB of rows, %d rows handed back by the keyed stream)" % (n_values, "first" if member_first else "last", n_bytes / 1e6, handed),
                      "  (a) bse_ingest_rows, keyed engine      %s" % med(t_keyed),
                      "      bse_ingest_rows, baseline engine   %s" % med(t_base),
                      "      removed from the caller's thread   %8.2f   bar (> combined spread %.2f): %s" % (
                          removed, spread(t_keyed) + spread(t_base), "MET" if removed > spread(t_keyed) + spread(t_base) else "NOT MET"),
                      "  (b) bsg_last_partition_ms, summed      %s" % med(p_ms),
                      "      bsg_last_minmax_ms, one call       %s   bar (partition <= minmax + its spread %.2f): %s" % (
                          med(m_ms), spread(m_ms), "MET" if statistics.median(p_ms) <= statistics.median(m_ms) + spread(m_ms) else "NOT MET"),
                      "      bsg_last_minmax_ms, same batches   %s   bar (partition <= minmax + its spread %.2f): %s" % (
                          med(mb_ms), spread(mb_ms), "MET" if statistics.median(p_ms) <= statistics.median(mb_ms) + spread(mb_ms) else "NOT MET"),
                      "  (c) ms_walk, keyed stream              %s" % med(w_keyed),
                      "      ms_walk, explicit sets (baseline)  %s   bar (equal within the spreads): %s" % (
                          med(w_plain), "MET" if abs(statistics.median(w_keyed) - statistics.median(w_plain)) <= spread(w_keyed) + spread(w_plain) else "NOT MET"), ""]
            print("\n".join(lines[-11:]), flush=True)
    text = "\n".join(lines) + "\n"
    if "--out" in opts:
        with open(opts["--out"], "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
