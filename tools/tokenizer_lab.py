"""Separator-family tokenizers on the device (bsg_ingest_rows_tok / bsg_match_rows_tok) on synth log rows: walk ms
(bsg_ingest_stats ms_walk, k_ingest_rows[_tok] dispatch time, best of R) and match ms (bsg_last_match_ms for
FieldToken(level, error) AND Token(cache), best of R) for the default calls, the default-plus-0x01 spec (the same words as the
default, so its cost over the default is the TokSpec scan's) and the punctuation spec; tokens emitted per row for each (from the
host mirror's tokenizer on the leaf texts of a sample of the rows), and walk time per emitted token.  Then the same for the
default spec with an n-gram width of 3 and of 4 (k_ingest_rows_gram / k_match_rows_gram): a window per rune instead of a token per
word, so also the distinct entries the walk left (summed over the sets) and how often a table had to grow (bsg_ingest_stats
table_grows: the walk is repeated after each).  Their match query is the substring form of the words' one: the AND of the windows
of "error" under level and of "cache" anywhere.

    python tools/tokenizer_lab.py [n_rows] [repeats]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import host as Hst, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
print("# python tools/tokenizer_lab.py %d %d — synth log rows, BSG_INGEST_TRUSTED_JSON, 10 000 rows per set; walk = bsg_ingest_stats\n"
      "# ms_walk (k_ingest_rows / k_ingest_rows_tok dispatch time), match = bsg_last_match_ms for And(FieldToken(level, error),\n"
      "# Token(cache)); best of %d.  tokens/row from the host mirror's tokenizer on a 20 000-row sample.  Bars: default + 0x01 walk\n"
      "# within 1.25x of the default; punctuation walk per token within 1.5x of the default's." % (n_rows, reps, reps))
print("rows %d, %.1f MB of row bytes" % (n_rows, int(off[-1]) / 1e6))

SPECS = [("default (bsg_ingest_rows / bsg_match_rows)", None),
         ("default + 0x01 (TokSpec kernels, same words)", Tokenizer(WHITE_SPACE + "\x01", unicode_space=True, lower=True)),
         ("punctuation \" \\t\\n\\v\\f\\r,;:=/.-\\\"[]()\" lowered", Tokenizer(" \t\n\v\f\r,;:=/.-\"[]()", unicode_space=True, lower=True)),
         ("default, trigrams (k_ingest_rows_gram, n = 3)", Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)),
         ("default, 4-grams (k_ingest_rows_gram, n = 4)", Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=4))]


def leaf_texts(v):
    """leafTokenInput of every leaf of a row parsed with parse_int / parse_float = str (numbers arrive as their literals)"""
    if isinstance(v, dict):
        for x in v.values():
            yield from leaf_texts(x)
    elif isinstance(v, list):
        for x in v:
            yield from leaf_texts(x)
    elif isinstance(v, str):
        yield v
    elif isinstance(v, bool):
        yield "true" if v else "false"


def tokens_per_row(spec, sample):
    n = 0
    for r in sample:
        obj = json.loads(r, parse_float=str, parse_int=str)
        for t in leaf_texts(obj):
            n += len(Hst.tokenize(t, spec))
    return n / len(sample)


per_set = 10_000
first = np.arange(0, n_rows + per_set, per_set, dtype=np.uint32)
first[-1] = n_rows
first = np.unique(first)
sample = rows[:: max(1, n_rows // 20000)]
base_walk = base_tok = None


def matcher_for(spec):
    """the words' query; under a width n its substring form (bloomgpu.h: AND the full n-rune windows of every needle word)"""
    n = spec.ngram if spec is not None else 0
    if not n:
        return Q.CompiledMatcher(Q.And(Q.FieldToken("level", "error"), Q.Token("cache")))
    grams = lambda w: [w[i:i + n] for i in range(len(w) - n + 1)]
    return Q.CompiledMatcher(Q.And(*[Q.FieldToken("level", g) for g in grams("error")], *[Q.Token(g) for g in grams("cache")]))


with Context((0,)) as ctx:
    for name, spec in SPECS:
        walk = 1e9
        for _ in range(reps + 1):                     # the first call warms the tables' pool
            ing = ctx.ingest_rows((blob, off), first, tokenizer=spec, flags=1)
            st = ctx.ingest_stats(ing)
            walk = min(walk, st.ms_walk)
            grows = st.table_grows                    # (the same every time: the tables start from the same sizes)
            counts, status = ctx.ingest_finish(ing, len(first) - 1)
            distinct = [int(x) for x in np.asarray(counts, dtype=np.int64).sum(axis=0)]
            ctx.ingest_free(ing)
        match = 1e9
        matcher = matcher_for(spec)
        ctx.match_rows((blob, off), matcher, tokenizer=spec)
        for _ in range(reps):
            hits, fb = ctx.match_rows((blob, off), matcher, tokenizer=spec)
            match = min(match, ctx.last_match_ms())
        tpr = tokens_per_row(spec, sample)
        ns_tok = walk * 1e6 / (tpr * n_rows)
        if base_walk is None:
            base_walk, base_tok = walk, ns_tok
        print("%-48s walk %7.3f ms (%.2fx)  match %6.3f ms  %5.2f tokens/row  %.3f ns walk per token (%.2fx)  %d hits %d fallback"
              "  table_grows %d  distinct fields/tokens/field::tokens %d/%d/%d (summed over %d sets)"
              % (name, walk, walk / base_walk, match, tpr, ns_tok, ns_tok / base_tok, int(hits.sum()), len(fb), grows, *distinct, len(first) - 1))
