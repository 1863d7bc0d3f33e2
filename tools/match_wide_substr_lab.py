"""One bsg_match_rows_wide_substr call against the ceil(Q / 64) bsg_match_rows_many_substr calls the same batch needs without it: synth
log rows in page-locked memory, under the default and the trigram spec, Q in {64, 256, 1024} queries over ONE table of 48 token
conditions (Token / FieldToken over the synth vocabulary) and 16 needles of 8 bytes (the whole 2 x 64 needle positions).  Query q is
And(two token conditions) AND an Or / And of two needles; every query is evaluated on every row (the implicit set: both results have
the batched call's plane layout, and at every Q the planes are compared bit for bit before anything is timed).
Both sides go through the C calls themselves with preallocated outputs.  The calls alternate (the batched calls of one round, then
the wide call), R rounds; per figure the median (min .. max) of the device time (bsg_last_match_ms: the walker launches, and for the
wide call its evaluation launch).  No ratio is fixed in advance: the last column only says whether the one call stayed below the SUM
of the calls it replaces.

    python tools/match_wide_substr_lab.py [n_rows] [rounds] [max_q]
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
# 16 needles of 8 bytes, each crossing a word boundary or lying inside a word of the synth vocabulary
NEEDLES = ["ion time", "che miss", "y reques", "ed cache", "ss shard", "database", "upstream", "rocessed", "ucceeded", "n failed", "d latenc", "hard ret",
           "region-7", "connecti", "t upstre", "eout ret"]
assert len(NEEDLES) == 16 and len(set(NEEDLES)) == 16 and all(len(n) == 8 for n in NEEDLES)


def token_conditions(spec):
    """48 distinct token conditions; under an n-gram spec a token is a word's last three runes (distinct over the vocabulary)"""
    t = (lambda s: s[-3:]) if spec is not None and spec.ngram else (lambda s: s)
    conds = [Q.FieldToken("level", t(x)) for x in synth.LEVELS] + [Q.FieldToken("service", t(x)) for x in synth.SERVICES]
    conds += [Q.FieldToken("nested.region", t("region-%d" % i)) for i in range(synth.N_REGIONS)]
    conds += [Q.Token(t(w)) for w in synth.WORDS] + [Q.FieldToken("tags", t(w)) for w in synth.WORDS] + [Q.FieldToken("message", t(w)) for w in synth.WORDS[:5]]
    assert len(conds) == 48
    return conds


def queries(spec, nq):
    conds = token_conditions(spec)
    rng = np.random.default_rng(20261020)
    out = []
    for q in range(nq):
        a, b = conds[q % 48], conds[int(rng.integers(0, 48))]
        n0, n1 = Q.Substring(NEEDLES[q % 16]), Q.Substring(NEEDLES[int(rng.integers(0, 16))])
        out.append(((Q.Or if q % 3 else Q.And)(a, b), None, (Q.SubstringOr if q % 2 else Q.SubstringAnd)(n0, n1)))
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
        rc = ctx.L.bsg_match_rows_many_substr(*self.head(ctx, data), None, None, 0, tok, p(self.out), p(self.fb), len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value)
        return ctx.last_match_ms()

    def wide(self, ctx, data, tok):
        p = _lib._ptr
        rc = ctx.L.bsg_match_rows_wide_substr(*self.head(ctx, data), None, None, None, 0, tok, self.out.ctypes.data, p(self.fb), len(self.fb), C.byref(self.nfb))
        assert rc == 0 and self.nfb.value == 0, (rc, self.nfb.value)
        return ctx.last_match_ms()


rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
print("# python tools/match_wide_substr_lab.py %d %d %d" % (n_rows, reps, max_q))
print("rows %d, %.1f MB of row bytes in page-locked memory; one table of 48 token conditions and 16 needles of 8 bytes; every query on every row"
      % (n_rows, n_bytes / 1e6))
print("device ms = bsg_last_match_ms, median (min .. max) of %d alternating rounds" % reps)
with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    data = (blob, off)
    for name, spec in (("default", None), ("trigram", TRIGRAM)):
        tok = None if spec is None else c_spec(spec)
        for nq in [q for q in (64, 256, 1024) if q <= max_q]:
            qs = queries(spec, nq)
            wide = Raw(Q.CompiledWideSubstringBatch(qs))
            groups = [Raw(Q.CompiledRowSubstringQueryBatch(qs[g: g + 64])) for g in range(0, nq, 64)]
            assert len(wide.kinds) == 64 and int((wide.kinds >= 4).sum()) == 16
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
            m, w = float(np.median(m_dev)), float(np.median(w_dev))
            print("%-8s Q=%4d  (query, row) matches %10d | %2d x bsg_match_rows_many_substr  %s ms | 1 x bsg_match_rows_wide_substr  %s ms | wide / sum %.3f%s"
                  % (name, nq, hits, len(groups), fmt(m_dev), fmt(w_dev), w / m, "" if nq < 128 else "  below the sum: %s" % ("yes" if w < m else "NO")))
            del wide, groups, planes
    ctx.pinned_free(blob)
