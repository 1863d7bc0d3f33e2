"""One bsg_match_rows_wide call against the ceil(Q / 64) bsg_match_rows_many calls the engine makes without DeviceMatchWide: synth
log rows in page-locked memory, in sets of 10 000 rows, Q in {64, 256, 1024, 4096} three-term And(FieldToken) queries of the bench's
C2 shape over its distinct level / service / nested.region terms.  A query is listed on the sets where an exact probe lets it
survive (every one of its three terms occurs in the set: with these terms that is every set, the dense end of the scale), and, as a
second scenario, on one set in ten (what a selective further term leaves).  At Q = 64 both calls also run with the implicit set
(every query on every row): what the split itself costs, the sat round trip through device memory and the second launch.
Both sides go through the C calls themselves with preallocated outputs (no unpacking of bits in Python on either side).
Per figure: wall ms, device ms (bsg_last_match_ms), median over R runs (min .. max), A and B back to back in the same process.
The wide call's device time is split by a second wide call over the same sets with ONE nil-program pair per listed set: the same
walk, next to no evaluation ("walk"); evaluation = total - walk.

    python tools/match_wide_lab.py [n_rows] [repeats] [max_q]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
max_q = int(args[2]) if len(args) > 2 else 4096
SET_ROWS = 10_000
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
d = synth.draws(0, n_rows)
dq = synth.draws(0, max_q)
exprs = [Q.And(Q.FieldToken("level", synth.LEVELS[dq["level"][i]]), Q.FieldToken("service", synth.SERVICES[dq["service"][i]]),
               Q.FieldToken("nested.region", "region-%d" % int(dq["region"][i]))) for i in range(max_q)]
first = list(range(0, n_rows, SET_ROWS)) + [n_rows]
n_sets = len(first) - 1
present = [tuple(set(int(x) for x in d[k][first[s]: first[s + 1]]) for k in ("level", "service", "region")) for s in range(n_sets)]
print("library %s\nrows %d in %d sets, %.1f MB of row bytes in page-locked memory, %d runs per figure: median (min .. max)"
      % (_lib.LIB_PATH, n_rows, n_sets, n_bytes / 1e6, reps))


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


def timed(fn):
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ms = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms)
    return wall, dev


import ctypes as C  # noqa: E402
from bloomsearch_amd.gpu import pack_entries  # noqa: E402


class Raw:
    """one batch's arguments for the C calls, built once; outputs allocated once"""

    def __init__(self, batch):
        self.cblob, self.coff = pack_entries([x for pair in zip(batch.fields, batch.tokens) for x in pair])
        self.kinds = np.asarray(batch.kinds, dtype=np.uint32)
        self.ops = np.asarray(batch.prog_ops, dtype=np.uint32)
        self.poff = np.asarray(batch.prog_off, dtype=np.uint32)
        self.nq = len(self.poff) - 1
        self.fb = np.zeros(n_rows, dtype=np.uint32)
        self.nfb = C.c_uint32()
        self.out = None

    def head(self, ctx, data):
        p = _lib._ptr
        return (ctx.h, p(data[0]), p(data[1]), n_rows, p(self.cblob), p(self.coff), p(self.kinds), len(self.kinds), p(self.ops), self.poff.ctypes.data, self.nq)

    def many(self, ctx, data, sfr, masks):
        if self.out is None:
            self.out = np.zeros(self.nq * ((n_rows + 63) // 64), dtype=np.uint64)
        p = _lib._ptr
        rc = ctx.L.bsg_match_rows_many(*self.head(ctx, data), p(sfr), p(masks), 0 if masks is None else len(masks), None, p(self.out), p(self.fb),
                                       len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, rc

    def wide(self, ctx, data, sfr, sqo, sq, total):
        if self.out is None or len(self.out) != total:
            self.out = np.zeros(total, dtype=np.uint64)
        p = _lib._ptr
        rc = ctx.L.bsg_match_rows_wide(*self.head(ctx, data), p(sfr), p(sqo), None if sq is None else sq.ctypes.data, 0 if sfr is None else len(sfr) - 1,
                                       None, self.out.ctypes.data, p(self.fb), len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, rc


def survives(q, s):
    return all(int(dq[k][q]) in present[s][i] for i, k in enumerate(("level", "service", "region")))


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    data = (blob, off)
    ctx.match_rows(data, Q.CompiledMatcher(exprs[0]))                              # warm: module load, scratch, lower table
    for nq in [q for q in (64, 256, 1024, 4096) if q <= max_q]:
        wide = Q.CompiledWideBatch(exprs[:nq])
        groups = [Q.CompiledMatcherBatch(exprs[g: g + 64]) for g in range(0, nq, 64)]
        raw_wide, raw_groups = Raw(wide), [Raw(b) for b in groups]
        first32 = np.asarray(first, dtype=np.uint32)
        for scenario in (["implicit"] if nq == 64 else []) + ["probe", "one set in ten"]:
            if scenario == "implicit":
                lists = None
            elif scenario == "probe":
                lists = [[q for q in range(nq) if survives(q, s)] for s in range(n_sets)]
            else:
                lists = [[q for q in range(nq) if (q + s) % 10 == 0 and survives(q, s)] for s in range(n_sets)]

            def run_wide():
                if lists is None:
                    raw_wide.wide(ctx, data, None, None, None, total_words)
                else:
                    raw_wide.wide(ctx, data, first32, sq_off, sq, total_words)
                return ctx.last_match_ms()

            def run_walk():                                                        # the same sets walked, one nil-program pair on each listed set
                ctx.match_rows_wide(data, nil_batch, first if lists is not None else [0, n_rows], walk_off, walk_q)
                return ctx.last_match_ms()

            def run_many():
                ms = 0.0
                for g, b in enumerate(raw_groups):
                    b.many(ctx, data, None if lists is None else first32, None if lists is None else masks[g])
                    ms += ctx.last_match_ms()
                return ms

            if lists is not None:
                sq_off = np.zeros(n_sets + 1, dtype=np.uint32)
                sq_off[1:] = np.cumsum([len(l) for l in lists])
                sq = np.asarray([q for l in lists for q in l], dtype=np.uint32)
                masks = [np.asarray([sum(1 << (q - g) for q in l if g <= q < g + 64) for l in lists], dtype=np.uint64) for g in range(0, nq, 64)]
                walk_off = np.cumsum([0] + [1 if l else 0 for l in lists]).astype(np.uint32)
                n_pairs = len(sq)
            else:
                walk_off, n_pairs = np.asarray([0, 1], dtype=np.uint32), nq
            walk_q = np.zeros(int(walk_off[-1]), dtype=np.uint32)
            nil_batch = Q.CompiledWideBatch([None])                              # one nil program, over the same condition table
            nil_batch.kinds, nil_batch.fields, nil_batch.tokens = wide.kinds, wide.fields, wide.tokens
            words, pwo, fb = (ctx.match_rows_wide(data, wide) if lists is None else ctx.match_rows_wide(data, wide, first, sq_off, sq))
            assert len(fb) == 0
            total_words = len(words)
            planes, _ = ctx.match_rows_many(data, groups[0]) if lists is None else ctx.match_rows_many(data, groups[0], first, masks[0])
            if lists is None:                                                      # the plane layout of the batched call, bit for bit
                n_words = (n_rows + 63) // 64
                got = np.unpackbits(words.view(np.uint8).reshape(nq, n_words * 8), axis=1, bitorder="little")[:, :n_rows].astype(bool)
                assert np.array_equal(got, planes)
            del planes
            # A / B back to back, twice: many, wide, walk, many, wide, walk
            m_wall, m_dev = timed(run_many)
            w_wall, w_dev = timed(run_wide)
            k_wall, k_dev = timed(run_walk)
            m2_wall, m2_dev = timed(run_many)
            w2_wall, w2_dev = timed(run_wide)
            m_wall, m_dev, w_wall, w_dev = m_wall + m2_wall, m_dev + m2_dev, w_wall + w2_wall, w_dev + w2_dev
            many_bytes = len(groups) * 64 * ((n_rows + 63) // 64) * 8 if nq >= 64 else 0
            print("Q=%4d %-14s pairs %7d  conditions %d" % (nq, scenario, n_pairs, len(wide.kinds)))
            print("   %3d x bsg_match_rows_many  wall ms %s   device ms %s   output %8.1f MB" % (len(groups), fmt(m_wall), fmt(m_dev), many_bytes / 1e6))
            print("     1 x bsg_match_rows_wide  wall ms %s   device ms %s   output %8.1f MB" % (fmt(w_wall), fmt(w_dev), len(words) * 8 / 1e6))
            print("         of which the walk    device ms %s   evaluation (total - walk) %.2f ms" % (fmt(k_dev), np.median(w_dev) - np.median(k_dev)))
            print("         wide / many: wall %.3f, device %.3f" % (np.median(w_wall) / np.median(m_wall), np.median(w_dev) / np.median(m_dev)))
            del words
    ctx.pinned_free(blob)
