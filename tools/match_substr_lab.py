"""Substring conditions on the device (bsg_match_rows_substr) on the rows tools/tokenizer_lab.py uses: synth log rows under the
trigram spec.  Device time (bsg_last_match_ms, best of R) of
  - bsg_match_rows_substr with 1, 8 and 16 any-field needles (an Or of Substring conditions: every row is walked, every needle steps
    on every text byte);
  - bsg_match_rows_tok over the same rows with the window-AND candidate query of the same needles (what a caller could do before);
  - for one field-scoped ASCII needle: bsg_match_rows_substr with FieldSubstring against bsg_match_rows_regex with the quoted literal;
and the share of rows where the window-AND candidate holds but the exact test does not.  No threshold: the numbers are the result.

    python tools/match_substr_lab.py [n_rows] [repeats]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import host as Hst, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SPEC = Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
print("# python tools/match_substr_lab.py %d %d — synth log rows, trigram spec; ms = bsg_last_match_ms (the walker launches of the call), best of %d"
      % (n_rows, reps, reps))
print("rows %d, %.1f MB of row bytes" % (n_rows, int(off[-1]) / 1e6))

# 16 needles of at most 8 bytes (128 needle bytes per call), each crossing a word boundary or lying inside a word of the synth vocabulary
NEEDLES = ["ion time", "che miss", "y reques", "eout", "pstrea", "ed cache", "atenc", "ss shard", "databa", "t retry", "ucceed", "n failed",
           "rocess", "d laten", "hard re", "gion-7"]


def best(fn):
    fn()
    ms = 1e9
    for _ in range(reps):
        out = fn()
        ms = min(ms, ctx.last_match_ms())
    return ms, out


def candidate(needle):
    """the window-AND candidate of one needle: its pruning terms as Token conditions"""
    terms = Hst.substring_terms(needle, SPEC)
    return Q.And(*[Q.Token(t) for t in terms]) if terms else None


with Context((0,)) as ctx:
    for k in (1, 8, 16):
        needles = NEEDLES[:k]
        exact = Q.CompiledSubstringQuery(None, Q.SubstringOr(*[Q.Substring(n) for n in needles]))
        ms_sub, (hits, fb) = best(lambda: ctx.match_rows_substr((blob, off), exact, SPEC))
        cands = [candidate(n) for n in needles]
        cand = Q.CompiledMatcher(None if any(c is None for c in cands) else Q.Or(*cands))
        ms_tok, (chits, cfb) = best(lambda: ctx.match_rows((blob, off), cand, tokenizer=SPEC))
        assert not (hits & ~chits).any(), "the candidate test lost a matching row"
        print("%2d any-field needles (%3d needle bytes, %2d candidate windows): bsg_match_rows_substr %7.3f ms, %d rows, %d fallback | "
              "window-AND candidate through bsg_match_rows_tok %7.3f ms, %d rows | candidate true, exact false: %d rows (%.3f%% of all)"
              % (k, sum(len(n) for n in needles), len(cand.kinds), ms_sub, int(hits.sum()), len(fb), ms_tok, int(chits.sum()),
                 int((chits & ~hits).sum()), 100.0 * int((chits & ~hits).sum()) / n_rows))
    needle = "ion time"                       # no regex metacharacter: the needle is its own quoted literal
    exact = Q.CompiledSubstringQuery(None, Q.FieldSubstring("message", needle))
    ms_sub, (hits, fb) = best(lambda: ctx.match_rows_substr((blob, off), exact, SPEC))
    rx = Q.CompiledRowQuery(None, Q.FieldRegex("message", needle))
    ms_rx, (rhits, rfb) = best(lambda: ctx.match_rows_regex((blob, off), rx, tokenizer=SPEC))
    assert np.array_equal(hits, rhits)
    print("FieldSubstring(message, %r): bsg_match_rows_substr %7.3f ms | bsg_match_rows_regex with the quoted literal %7.3f ms | %d rows both"
          % (needle, ms_sub, ms_rx, int(hits.sum())))
