"""One bsg_match_rows_lookup_rows call against the bsg_match_rows_wide_rows calls the same batch needs when it is cut into tables of 64
conditions: synth log rows in page-locked memory in 100 sets, every query listed on every set, needle queries
FieldToken("user_id", u) on distinct user ids of the rows (a batch of standing searches: as many distinct conditions as queries).
  (a) Q = 1 024: one lookup call against 16 wide calls       (b) Q = 256: one against 4
  (c) a 64-condition table with ONE single-term query (the evaluation is next to nothing): the lookup walker's device time against
      k_match_rows_store's, the price of the lookup where the loop over the table still fits
Both sides go through the C calls with preallocated outputs; the wide side's figures are the sums over its calls.  Every side's
lists are compared before anything is timed.  Alternating rounds in one session: A, B, A, B, ... reps times each.  Per figure:
median (min .. max) of the wall ms of the call(s), the device ms (bsg_last_match_ms) and the bytes returned.

    python tools/match_lookup_lab.py [n_rows] [repeats]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, pack_entries  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
N_SETS = 100
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
uids = []
for u in synth.draws(0, min(n_rows, 200_000))["user_id"]:
    if int(u) not in uids:
        uids.append(int(u))
    if len(uids) == 1024:
        break
assert len(uids) == 1024, "the rows hold fewer than 1 024 distinct user ids"
needle = [Q.FieldToken("user_id", str(u)) for u in uids]
first = np.asarray([n_rows * s // N_SETS for s in range(N_SETS + 1)], dtype=np.uint32)
print("library %s\nrows %d in %d sets, %.1f MB of row bytes in page-locked memory, %d alternating rounds per figure: median (min .. max)"
      % (_lib.LIB_PATH, n_rows, N_SETS, n_bytes / 1e6, reps))


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


class Call:
    """one C call over `exprs` on every set, its outputs preallocated"""

    def __init__(self, ctx, blob, name, exprs, rows_call=True):
        self.ctx, self.fn, self.rows_call = ctx, getattr(ctx.L, name), rows_call
        batch = (Q.CompiledLookupBatch if "lookup" in name else Q.CompiledWideBatch)(exprs)
        nq = batch.n_queries
        p = _lib._ptr
        cblob, coff = pack_entries([x for pair in zip(batch.fields, batch.tokens) for x in pair])
        kinds, ops, poff = (np.asarray(a, dtype=np.uint32) for a in (batch.kinds, batch.prog_ops, batch.prog_off))
        sqo = np.arange(N_SETS + 1, dtype=np.uint32) * np.uint32(nq)
        sq = np.tile(np.arange(nq, dtype=np.uint32), N_SETS)
        self.n_pairs, self.nq, self.n_conds = len(sq), nq, len(kinds)
        _, total = ctx.match_wide_size(first, sqo, n_rows, nq)
        self.keep = (cblob, coff, kinds, ops, poff, sqo, sq)
        self.head = (ctx.h, p(blob), p(off), n_rows, p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq, p(first), p(sqo), sq.ctypes.data,
                     N_SETS, None)
        self.words = np.zeros(0 if rows_call else total, dtype=np.uint64)
        self.hdr, self.pair_off = np.zeros(self.n_pairs, dtype=np.uint32), np.zeros(self.n_pairs + 1, dtype=np.uint64)
        self.payload = np.zeros(2 * total if rows_call else 0, dtype=np.uint32)
        self.fb, self.nfb, self.plen = np.zeros(n_rows, dtype=np.uint32), C.c_uint32(), C.c_uint64()

    def run(self):
        """-> (wall ms, device ms, bytes returned)"""
        p = _lib._ptr
        t0 = time.perf_counter()
        if self.rows_call:
            rc = self.fn(*self.head, self.hdr.ctypes.data, self.pair_off.ctypes.data, self.payload.ctypes.data, len(self.payload), C.byref(self.plen),
                         p(self.fb), len(self.fb), C.byref(self.nfb))
        else:
            rc = self.fn(*self.head, self.words.ctypes.data, p(self.fb), len(self.fb), C.byref(self.nfb))
        t1 = time.perf_counter()
        assert rc == 0 and self.nfb.value == 0, (rc, self.ctx.L.bsg_last_error(self.ctx.h))
        return (t1 - t0) * 1e3, self.ctx.last_match_ms(), (self.n_pairs * 4 + self.plen.value * 4) if self.rows_call else len(self.words) * 8

    def lists(self):
        """per (set, query): the pair's header and payload"""
        h = self.hdr.reshape(N_SETS, self.nq)
        return h, [[self.payload[int(self.pair_off[s * self.nq + q]): int(self.pair_off[s * self.nq + q + 1])].copy() for q in range(self.nq)] for s in range(N_SETS)]


def summed(calls):
    r = [c.run() for c in calls]
    return tuple(sum(x[i] for x in r) for i in range(3))


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    ctx.match_rows((blob, off), Q.CompiledMatcher(needle[0]))                      # warm: module load, scratch, lower table
    for label, nq in (("(a)", 1024), ("(b)", 256)):
        lookup = [Call(ctx, blob, "bsg_match_rows_lookup_rows", needle[:nq])]
        wide = [Call(ctx, blob, "bsg_match_rows_wide_rows", needle[g: g + 64]) for g in range(0, nq, 64)]
        summed(lookup), summed(wide)                                               # warm, and both sides hold the same lists
        lh, lp = lookup[0].lists()
        matches = 0
        for g, w in enumerate(wide):
            wh, wp = w.lists()
            assert np.array_equal(lh[:, g * 64: g * 64 + 64], wh)
            for s in range(N_SETS):
                for q in range(64):
                    assert np.array_equal(lp[s][g * 64 + q], wp[s][q])
                    matches += len(wp[s][q])
        res = {"lookup": [], "wide": []}
        for _ in range(reps):
            res["lookup"].append(summed(lookup))
            res["wide"].append(summed(wide))
        print("%s Q=%4d distinct conditions %d, pairs %d, listed rows %d: 1 bsg_match_rows_lookup_rows call against %d bsg_match_rows_wide_rows calls"
              % (label, nq, lookup[0].n_conds, lookup[0].n_pairs, matches, len(wide)))
        for name in ("lookup", "wide"):
            wall, dev, nbytes = zip(*res[name])
            print("   %-6s  wall ms %s   device ms %s   returned %9.3f MB" % (name, fmt(wall), fmt(dev), nbytes[0] / 1e6))
        med = {k: [float(np.median([r[i] for r in v])) for i in range(2)] for k, v in res.items()}
        print("   wide / lookup: wall %.2f, device %.2f" % (med["wide"][0] / med["lookup"][0], med["wide"][1] / med["lookup"][1]))
        del lookup, wide
    table = needle[:64]
    calls = {}
    for name in ("bsg_match_rows_lookup", "bsg_match_rows_wide"):
        c = Call(ctx, blob, name, table, rows_call=False)
        # ONE query over the 64-condition table: the walk collects all 64 flags, the evaluation reads one
        c.keep[3][:] = 0
        poff = np.asarray([0, 1], dtype=np.uint32)
        sqo = np.arange(N_SETS + 1, dtype=np.uint32)
        sq = np.zeros(N_SETS, dtype=np.uint32)
        _, total = ctx.match_wide_size(first, sqo, n_rows, 1)
        head = list(c.head)
        head[9], head[10], head[12], head[13] = poff.ctypes.data, 1, _lib._ptr(sqo), sq.ctypes.data
        c.head, c.words, c.n_pairs, c.nq = tuple(head), np.zeros(total, dtype=np.uint64), N_SETS, 1
        c.keep += (poff, sqo, sq)
        calls[name] = c
        c.run()
    assert calls["bsg_match_rows_lookup"].words.tobytes() == calls["bsg_match_rows_wide"].words.tobytes()
    res = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            res[k].append(c.run())
    print("(c) a 64-condition table, one single-term query: the walk (and an evaluation of one op per row)")
    for k, v in res.items():
        wall, dev, nbytes = zip(*v)
        print("   %-22s wall ms %s   device ms %s" % (k, fmt(wall), fmt(dev)))
    print("   lookup / wide: device %.3f" % (np.median([r[1] for r in res["bsg_match_rows_lookup"]]) / np.median([r[1] for r in res["bsg_match_rows_wide"]])))
    ctx.pinned_free(blob)
