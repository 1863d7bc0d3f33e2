"""One bsg_match_rows_lookup_regex_rows call against the bsg_match_rows_wide_rows calls the same batch needs when it is cut into tables
of 64 conditions: synth log rows in page-locked memory in 100 sets, every query listed on every set.
  (a) 1 008 needle queries FieldToken("user_id", u) on distinct user ids of the rows plus 16 regex-only queries, two on each of the
      rows' eight leaf fields (so at most two DFAs are open on a leaf): one lookup-regex call against 16 wide calls, the last of
      which holds the 16 regex conditions
  (b) a 64-condition table, 60 needle conditions and 4 regex conditions on four fields, with ONE query, the Or of the four regex
      conditions (every set's mask selects all four, the evaluation is seven ops per row): the new walker's device time against
      k_match_rows_store_regex's, the price of the lookup where the loop over the table still fits
Both sides go through the C calls with preallocated outputs; the wide side's figures are the sums over its calls.  Every side's
lists are compared before anything is timed.  Alternating rounds in one session: A, B, A, B, ... reps times each.  Per figure:
median (min .. max) of the wall ms of the call(s), the device ms (bsg_last_match_ms) and the bytes returned.  The lines go to
stdout and to profiles/match_lookup_regex_lab.txt.

    python tools/match_lookup_regex_lab.py [n_rows] [repeats]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, pack_entries  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 3
N_SETS = 100
REGEX = [("level", "^err"), ("level", "^(warn|info)"), ("message", "timeout|cache"), ("message", "retry.*failed"), ("nested.az", "^az-1$"),
         ("nested.az", "az-[02]"), ("nested.region", "region-[37]$"), ("nested.region", "^region-1"), ("service", "^pay"), ("service", "gate|bill"),
         ("tags", "^latency$"), ("tags", "up.*am"), ("timestamp", "00$"), ("timestamp", "^17000000[0-4]"), ("user_id", "^1[0-9]+7$"),
         ("user_id", "^[0-9]{4}$")]
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
uids = []
for u in synth.draws(0, min(n_rows, 200_000))["user_id"]:
    if int(u) not in uids:
        uids.append(int(u))
    if len(uids) == 1008:
        break
assert len(uids) == 1008, "the rows hold fewer than 1 008 distinct user ids"
needle = [Q.FieldToken("user_id", str(u)) for u in uids]
regex = [(None, Q.FieldRegex(f, p)) for f, p in REGEX]
first = np.asarray([n_rows * s // N_SETS for s in range(N_SETS + 1)], dtype=np.uint32)
lines = []


def out(text):
    print(text, flush=True)
    lines.append(text)


out("library %s\nrows %d in %d sets, %.1f MB of row bytes in page-locked memory, %d alternating rounds per figure: median (min .. max)"
    % (os.path.relpath(_lib.LIB_PATH, ROOT), n_rows, N_SETS, n_bytes / 1e6, reps))


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


class Call:
    """one C call over `items` (or a ready batch) on every set, its outputs preallocated"""

    def __init__(self, ctx, blob, name, items, rows_call=True, batch=None):
        self.ctx, self.fn, self.rows_call = ctx, getattr(ctx.L, name), rows_call
        batch = batch or (Q.CompiledLookupRegexBatch if "lookup" in name else Q.CompiledWideBatch)(items)
        nq = len(batch.prog_off) - 1
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
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value, self.ctx.L.bsg_last_error(self.ctx.h))
        return (t1 - t0) * 1e3, self.ctx.last_match_ms(), (self.n_pairs * 4 + self.plen.value * 4) if self.rows_call else len(self.words) * 8

    def lists(self):
        """per (set, query): the pair's header and payload"""
        h = self.hdr.reshape(N_SETS, self.nq)
        return h, [[self.payload[int(self.pair_off[s * self.nq + q]): int(self.pair_off[s * self.nq + q + 1])].copy() for q in range(self.nq)] for s in range(N_SETS)]


def summed(calls):
    r = [c.run() for c in calls]
    return tuple(sum(x[i] for x in r) for i in range(3))


class OneQuery:
    """60 needle conditions and 4 regex conditions, one query: the Or of the four regex conditions"""

    def __init__(self):
        four = [REGEX[2], REGEX[8], REGEX[0], REGEX[6]]                              # message, service, level, nested.region
        self.kinds = [_lib.KIND_FIELD_TOKEN] * 60 + [_lib.KIND_FIELD_REGEX] * 4
        self.fields = [b"user_id"] * 60 + [f.encode() for f, _ in four]
        self.tokens = [str(u).encode() for u in uids[:60]] + [p.encode() for _, p in four]
        self.prog_ops = [_lib.op(_lib.OP_TERM, 60 + k) for k in range(4)] + [_lib.op(_lib.OP_OR, 4)]
        self.prog_off = [0, len(self.prog_ops)]


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    ctx.match_rows((blob, off), Q.CompiledMatcher(needle[0]))                      # warm: module load, scratch, lower table
    items = needle + regex
    lookup = [Call(ctx, blob, "bsg_match_rows_lookup_regex_rows", items)]
    wide = [Call(ctx, blob, "bsg_match_rows_wide_rows", items[g: g + 64]) for g in range(0, len(items), 64)]
    summed(lookup), summed(wide)                                                   # warm, and both sides hold the same lists
    lh, lp = lookup[0].lists()
    matches = 0
    for g, w in enumerate(wide):
        wh, wp = w.lists()
        assert np.array_equal(lh[:, g * 64: g * 64 + 64], wh)
        for s in range(N_SETS):
            for q in range(w.nq):
                assert np.array_equal(lp[s][g * 64 + q], wp[s][q])
                matches += len(wp[s][q])
    res = {"lookup": [], "wide": []}
    for _ in range(reps):
        res["lookup"].append(summed(lookup))
        res["wide"].append(summed(wide))
    out("(a) Q=%4d: %d distinct conditions, %d of them regex, pairs %d, listed rows %d: 1 bsg_match_rows_lookup_regex_rows call against %d bsg_match_rows_wide_rows calls"
        % (len(items), lookup[0].n_conds, len(regex), lookup[0].n_pairs, matches, len(wide)))
    for name in ("lookup", "wide"):
        wall, dev, nbytes = zip(*res[name])
        out("   %-6s  wall ms %s   device ms %s   returned %9.3f MB" % (name, fmt(wall), fmt(dev), nbytes[0] / 1e6))
    med = {k: [float(np.median([r[i] for r in v])) for i in range(2)] for k, v in res.items()}
    out("   wide / lookup: wall %.2f, device %.2f" % (med["wide"][0] / med["lookup"][0], med["wide"][1] / med["lookup"][1]))
    del lookup, wide
    calls = {name: Call(ctx, blob, name, None, rows_call=False, batch=OneQuery()) for name in ("bsg_match_rows_lookup_regex", "bsg_match_rows_wide")}
    for c in calls.values():
        c.run()
    assert calls["bsg_match_rows_lookup_regex"].words.tobytes() == calls["bsg_match_rows_wide"].words.tobytes()
    res = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            res[k].append(c.run())
    out("(b) a 64-condition table with 4 regex conditions, one query (their Or): the walk (and an evaluation of seven ops per row)")
    for k, v in res.items():
        wall, dev, nbytes = zip(*v)
        out("   %-28s wall ms %s   device ms %s" % (k, fmt(wall), fmt(dev)))
    out("   lookup regex / wide: device %.3f" % (np.median([r[1] for r in res["bsg_match_rows_lookup_regex"]]) / np.median([r[1] for r in res["bsg_match_rows_wide"]])))
    ctx.pinned_free(blob)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "match_lookup_regex_lab.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
