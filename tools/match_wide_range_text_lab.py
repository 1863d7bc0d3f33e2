"""One bsg_match_rows_wide_regex_substr_range call over a batch of Q mixed queries (a time window beside a text search) against what the
same batch costs without it: synth log rows in page-locked memory, under the default and the trigram spec, Q in {16, 64, 256} queries
over ONE table of 12 token conditions, 4 regex conditions, 8 needles and 16 range conditions (8 windows of `timestamp`, 8 of `user_id`).
Query q is And(a token condition or nothing, a regex condition or nothing, a needle, a range condition); every query is evaluated on every
row (the implicit set: the wide result has the batched call's plane layout), and at every Q the planes are compared bit for bit with the
batched calls' - and at Q = 16 with every single call's - before anything is timed.
  (a) the one call | the Q bsg_match_rows_regex_substr_range calls the engine mirror makes today under a wide key, each with the table of
      its own query: one upload and one walk of the same rows per query
  (b) the one call | the ceil(Q / 64) bsg_match_rows_many_regex_substr_range calls of the same batch
  (c) the one call | bsg_match_rows_wide_substr (k_match_rows_store_regex_substr*) over the same table and programs with the range
      conditions removed: what the number consumer costs in the storing walker
All sides go through the C calls themselves with preallocated outputs.  The sides alternate within a round, R rounds after one warm-up
round; per figure the median (min .. max) of the device time (bsg_last_match_ms: the walker launches, and for a wide call its evaluation
launch) and the median of the wall time of the calls (upload included).  No threshold is set: the figures are recorded as they come.

    python tools/match_wide_range_text_lab.py [n_rows] [rounds] [out_file]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, c_spec, pack_entries  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "match_wide_range_text_lab.txt")
TRIGRAM = Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)
T0 = synth.TS_BASE                                               # synth: row i has timestamp T0 + i
REGEXES = [None, Q.FieldRegex("message", "timeout|cache"), Q.FieldRegex("service", "^(auth|pay)"), Q.FieldRegex("nested.region", "region-[37]$"),
           Q.FieldRegex("level", "(?i)error")]
NEEDLES = [Q.Substring(n) for n in ("ion time", "che miss", "y reques", "eout")] + [Q.FieldSubstring("message", n) for n in ("pstrea", "ed cache", "atenc", "ss shard")]
RANGES = [Q.FieldRange("timestamp", T0 + k * (n_rows // 8), T0 + k * (n_rows // 8) + n_rows // 4, hi_open=bool(k % 2)) for k in range(8)] + \
         [Q.FieldRange("user_id", 10000 * k, 10000 * k + 25000, lo_open=bool(k % 2)) for k in range(8)]


def token_conditions(spec):
    """12 distinct token conditions (and nothing); under an n-gram spec a token is a word's last three runes"""
    t = (lambda s: s[-3:]) if spec is not None and spec.ngram else (lambda s: s)
    return [None] + [Q.FieldToken("level", t(x)) for x in synth.LEVELS[:4]] + [Q.FieldToken("service", t(x)) for x in synth.SERVICES[:4]] + \
           [Q.Token(t(w)) for w in synth.WORDS[:4]]


def queries(spec, nq):
    """nq distinct mixed queries: every one holds a range condition beside a text condition"""
    tokens = token_conditions(spec)
    rng = np.random.default_rng(20261021)
    out, seen = [], set()
    while len(out) < nq:
        key = (int(rng.integers(0, len(tokens))) if len(out) % 2 else 0, len(out) % len(REGEXES), int(rng.integers(0, len(NEEDLES))), int(rng.integers(0, len(RANGES))))
        if key in seen:
            continue
        seen.add(key)
        out.append((tokens[key[0]], REGEXES[key[1]], NEEDLES[key[2]], RANGES[key[3]]))
    return out


def fmt(v):
    return "%9.2f (%9.2f .. %9.2f)" % (float(np.median(v)), min(v), max(v))


FALLBACK, N_FALLBACK = np.zeros(n_rows, dtype=np.uint32), C.c_uint32()


class Raw:
    """one table's arguments for the C calls, built once; the output allocated once"""

    def __init__(self, batch, single=False):
        self.cblob, self.coff = pack_entries([x for pair in zip(batch.fields, batch.tokens) for x in pair])
        self.kinds = np.asarray(batch.kinds, dtype=np.uint32)
        self.ops = np.asarray(batch.prog_ops, dtype=np.uint32)
        self.poff = None if single else np.asarray(batch.prog_off, dtype=np.uint32)
        self.nq = 1 if single else len(self.poff) - 1
        self.fb, self.nfb = FALLBACK, N_FALLBACK                     # shared: no call of the lab hands a row back
        self.out = np.zeros(self.nq * ((n_rows + 63) // 64), dtype=np.uint64)

    def head(self, ctx, data):
        p = _lib._ptr
        return (ctx.h, p(data[0]), p(data[1]), n_rows, p(self.cblob), p(self.coff), p(self.kinds), len(self.kinds), p(self.ops))

    def done(self, ctx, rc):
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value)
        return ctx.last_match_ms()

    def single(self, ctx, data, tok):
        p = _lib._ptr
        return self.done(ctx, ctx.L.bsg_match_rows_regex_substr_range(*self.head(ctx, data), len(self.ops), tok, p(self.out), p(self.fb), len(self.fb), C.byref(self.nfb)))

    def many(self, ctx, data, tok):
        p = _lib._ptr
        return self.done(ctx, ctx.L.bsg_match_rows_many_regex_substr_range(*self.head(ctx, data), self.poff.ctypes.data, self.nq, None, None, 0, tok, p(self.out), p(self.fb),
                                                                          len(self.fb), C.byref(self.nfb)))

    def wide(self, ctx, data, tok, call="bsg_match_rows_wide_regex_substr_range"):
        p = _lib._ptr
        return self.done(ctx, getattr(ctx.L, call)(*self.head(ctx, data), self.poff.ctypes.data, self.nq, None, None, None, 0, tok, self.out.ctypes.data, p(self.fb),
                                                   len(self.fb), C.byref(self.nfb)))


def timed(fn):
    t = time.perf_counter()
    dev = fn()
    return dev, (time.perf_counter() - t) * 1e3


rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
lines = ["# python tools/match_wide_range_text_lab.py %d %d" % (n_rows, reps),
         "rows %d, %.1f MB of row bytes in page-locked memory; one table of up to 12 token conditions, 4 regex conditions, 8 needles and 16 range conditions (what the Q queries use); every query on every row"
         % (n_rows, n_bytes / 1e6),
         "device ms = bsg_last_match_ms summed over a side's calls, median (min .. max) of %d alternating rounds after one warm-up round; wall ms = the same calls timed on the host, median"
         % reps]
print("\n".join(lines), flush=True)
with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    data = (blob, off)
    for name, spec in (("default", None), ("trigram", TRIGRAM)):
        tok = None if spec is None else c_spec(spec)
        for nq in (16, 64, 256):
            qs = queries(spec, nq)
            wide = Raw(Q.CompiledWideTextRangeBatch(qs))
            text = Raw(Q.CompiledWideSubstringBatch([(b, r, s) for b, r, s, _ in qs]))
            groups = [Raw(Q.CompiledRowTextRangeQueryBatch(qs[g: g + 64])) for g in range(0, nq, 64)]
            singles = [Raw(Q.CompiledRowTextRangeQuery(*quad), single=True) for quad in qs]
            assert int((wide.kinds == _lib.KIND_FIELD_RANGE).sum()) > 0 and int((text.kinds == _lib.KIND_FIELD_RANGE).sum()) == 0
            assert len(text.kinds) == len(wide.kinds) - int((wide.kinds == _lib.KIND_FIELD_RANGE).sum())
            # the same bits first (this is also the warm-up round of every side)
            wide.wide(ctx, data, tok)
            planes = wide.out.reshape(nq, -1)
            hits = int(np.unpackbits(wide.out.view(np.uint8)).sum())
            for g, b in enumerate(groups):
                b.many(ctx, data, tok)
                assert np.array_equal(b.out.reshape(b.nq, -1), planes[g * 64: g * 64 + b.nq]), (name, nq, g)
            for q, s in enumerate(singles):
                s.single(ctx, data, tok)
                assert nq > 16 or np.array_equal(s.out, planes[q]), (name, nq, q)
            text.wide(ctx, data, tok, "bsg_match_rows_wide_substr")
            assert not (planes & ~text.out.reshape(nq, -1)).any(), (name, nq)   # the text side alone matches at least the mixed query's rows
            dev = {k: [] for k in ("wide", "single", "many", "text")}
            wall = {k: [] for k in dev}
            for _ in range(reps):
                for k, fn in (("single", lambda: sum(s.single(ctx, data, tok) for s in singles)), ("many", lambda: sum(b.many(ctx, data, tok) for b in groups)),
                              ("wide", lambda: wide.wide(ctx, data, tok)), ("text", lambda: text.wide(ctx, data, tok, "bsg_match_rows_wide_substr"))):
                    d, w = timed(fn)
                    dev[k].append(d)
                    wall[k].append(w)
            med = {k: float(np.median(v)) for k, v in dev.items()}
            wmed = {k: float(np.median(v)) for k, v in wall.items()}
            head = "%-8s Q=%3d %2d conditions, (query, row) matches %10d" % (name, nq, len(wide.kinds), hits)
            out = [
                "%s | (a) 1 x bsg_match_rows_wide_regex_substr_range %s ms device, %9.2f ms wall | %3d x bsg_match_rows_regex_substr_range %s ms device, %9.2f ms wall | "
                "wide / sum %.3f device, %.3f wall" % (head, fmt(dev["wide"]), wmed["wide"], nq, fmt(dev["single"]), wmed["single"], med["wide"] / med["single"],
                                                       wmed["wide"] / wmed["single"]),
                "%s | (b) 1 x bsg_match_rows_wide_regex_substr_range %s ms device, %9.2f ms wall | %3d x bsg_match_rows_many_regex_substr_range %s ms device, %9.2f ms wall | "
                "wide / sum %.3f device, %.3f wall" % (head, fmt(dev["wide"]), wmed["wide"], len(groups), fmt(dev["many"]), wmed["many"], med["wide"] / med["many"],
                                                       wmed["wide"] / wmed["many"]),
                "%s | (c) k_match_rows_store_regex_substr_range + evaluation %s ms device | k_match_rows_store_regex_substr + evaluation, the %d range conditions removed "
                "%s ms device | with / without %.3f" % (head, fmt(dev["wide"]), len(wide.kinds) - len(text.kinds), fmt(dev["text"]), med["wide"] / med["text"]),
            ]
            for line in out:
                print(line, flush=True)
            lines += out
            del wide, text, groups, singles, planes
    ctx.pinned_free(blob)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
