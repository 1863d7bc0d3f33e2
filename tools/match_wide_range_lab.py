"""One bsg_match_rows_wide_range call against the ceil(Q / 64) bsg_match_rows_many_range calls the same batch needs without it: synth log
rows in page-locked memory, under the default and the trigram spec, Q in {64, 256, 1024} queries over ONE table of 48 token conditions
(Token / FieldToken over the synth vocabulary) and 16 range conditions on `timestamp` (windows of the rows' own timestamps: closed,
open and half-bounded).  Query q is an Or / And of two token conditions AND an Or / And of two range conditions; every query is
evaluated on every row (the implicit set: both results have the batched call's plane layout, and at every Q the planes are compared
bit for bit before anything is timed).
Both sides go through the C calls themselves with preallocated outputs.  The calls alternate (the batched calls of one round, then
the wide call), R rounds; per figure the median (min .. max) of the device time (bsg_last_match_ms: the walker launches, and for the
wide call its evaluation launch).  No ratio is fixed in advance.  For Q >= 128 the last column says whether the one call stayed below
the SUM of the calls it replaces by more than the spread (max - min) the rounds of the replaced side show.

    python tools/match_wide_range_lab.py [n_rows] [rounds] [max_q]
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, c_spec, pack_entries  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
max_q = int(args[2]) if len(args) > 2 else 1024
TRIGRAM = Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)


def range_conditions():
    """16 distinct range conditions on timestamp over the rows' own span: twelve windows of a sixteenth of it, four half-bounded"""
    t0, step = synth.TS_BASE, max(n_rows // 16, 1)
    conds = [Q.FieldRange("timestamp", t0 + i * step, t0 + (i + 1) * step, lo_open=bool(i % 2), hi_open=bool(i % 3)) for i in range(12)]
    conds += [Q.FieldRange("timestamp", t0 + 13 * step, None), Q.FieldRange("timestamp", None, t0 + 2 * step, hi_open=True),
              Q.FieldRange("timestamp", t0 + 15 * step, None, lo_open=True), Q.FieldRange("timestamp", None, t0 + step // 2)]
    assert len(conds) == 16 and len({Q.range_entry(c["Condition"]) for c in conds}) == 16
    return conds


def token_conditions(spec):
    """48 distinct token conditions; under an n-gram spec a token is a word's last three runes (distinct over the vocabulary)"""
    t = (lambda s: s[-3:]) if spec is not None and spec.ngram else (lambda s: s)
    conds = [Q.FieldToken("level", t(x)) for x in synth.LEVELS] + [Q.FieldToken("service", t(x)) for x in synth.SERVICES]
    conds += [Q.FieldToken("nested.region", t("region-%d" % i)) for i in range(synth.N_REGIONS)]
    conds += [Q.Token(t(w)) for w in synth.WORDS] + [Q.FieldToken("tags", t(w)) for w in synth.WORDS] + [Q.FieldToken("message", t(w)) for w in synth.WORDS[:5]]
    assert len(conds) == 48
    return conds


def queries(spec, nq):
    conds, ranges = token_conditions(spec), range_conditions()
    rng = np.random.default_rng(20261020)
    out = []
    for q in range(nq):
        a, b = conds[q % 48], conds[int(rng.integers(0, 48))]
        r0, r1 = ranges[q % 16], ranges[int(rng.integers(0, 16))]
        out.append(((Q.Or if q % 3 else Q.And)(a, b), (Q.RangeOr if q % 2 else Q.RangeAnd)(r0, r1)))
    return out


def fmt(v):
    return "%8.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


class Raw:
    """one batch's arguments for the C calls, built once; the output allocated once"""

    def __init__(self, batch):
        self.cblob, self.coff = pack_entries([x for pair in zip(batch.fields, batch.tokens) for x in pair])
        self.kinds = np.asarray(batch.kinds, dtype=np.uint32)
        self.ops = np.asarray(batch.prog_ops, dtype=np.uint32)
        self.poff = np.asarray(batch.prog_off, dtype=np.uint32)
        self.nq = len(self.poff) - 1
        self.fb = np.zeros(n_rows, dtype=np.uint32)
        self.nfb = C.c_uint32()
        self.out = np.zeros(self.nq * ((n_rows + 63) // 64), dtype=np.uint64)

    def head(self, ctx, data):
        p = _lib._ptr
        return (ctx.h, p(data[0]), p(data[1]), n_rows, p(self.cblob), p(self.coff), p(self.kinds), len(self.kinds), p(self.ops), self.poff.ctypes.data, self.nq)

    def many(self, ctx, data, tok):
        p = _lib._ptr
        rc = ctx.L.bsg_match_rows_many_range(*self.head(ctx, data), None, None, 0, tok, p(self.out), p(self.fb), len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value)
        return ctx.last_match_ms()

    def wide(self, ctx, data, tok):
        p = _lib._ptr
        rc = ctx.L.bsg_match_rows_wide_range(*self.head(ctx, data), None, None, None, 0, tok, self.out.ctypes.data, p(self.fb), len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value)
        return ctx.last_match_ms()


rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
print("# python tools/match_wide_range_lab.py %d %d %d" % (n_rows, reps, max_q))
print("rows %d, %.1f MB of row bytes in page-locked memory; one table of 48 token conditions and 16 range conditions on timestamp; every query on every row"
      % (n_rows, n_bytes / 1e6))
print("device ms = bsg_last_match_ms, median (min .. max) of %d alternating rounds; margin = max - min of the replaced side's rounds" % reps)
with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    data = (blob, off)
    for name, spec in (("default", None), ("trigram", TRIGRAM)):
        tok = None if spec is None else c_spec(spec)
        for nq in [q for q in (64, 256, 1024) if q <= max_q]:
            qs = queries(spec, nq)
            wide = Raw(Q.CompiledWideRangeBatch(qs))
            groups = [Raw(Q.CompiledRangeQueryBatch(qs[g: g + 64])) for g in range(0, nq, 64)]
            assert len(wide.kinds) == 64 and int((wide.kinds == _lib.KIND_FIELD_RANGE).sum()) == 16
            # the same bits first (this also warms both paths)
            wide.wide(ctx, data, tok)
            planes = wide.out.reshape(nq, -1)
            hits = 0
            for g, b in enumerate(groups):
                b.many(ctx, data, tok)
                assert np.array_equal(b.out.reshape(b.nq, -1), planes[g * 64: g * 64 + b.nq]), (name, nq, g)
                hits += int(np.unpackbits(b.out.view(np.uint8)).sum())
            m_dev, w_dev = [], []
            for _ in range(reps):
                m_dev.append(sum(b.many(ctx, data, tok) for b in groups))
                w_dev.append(wide.wide(ctx, data, tok))
            m, w, margin = float(np.median(m_dev)), float(np.median(w_dev)), max(m_dev) - min(m_dev)
            print("%-8s Q=%4d  (query, row) matches %10d | %2d x bsg_match_rows_many_range  %s ms | 1 x bsg_match_rows_wide_range  %s ms | wide / sum %.3f%s"
                  % (name, nq, hits, len(groups), fmt(m_dev), fmt(w_dev), w / m,
                     "" if nq < 128 else "  margin %.2f ms, below the sum by more: %s" % (margin, "yes" if w < m - margin else "NO")))
            del wide, groups, planes
    ctx.pinned_free(blob)
