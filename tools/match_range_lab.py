"""Range conditions on the device (bsg_match_rows_range) on 1 M synth log rows, under the default and the trigram spec.  Kernel time
(bsg_last_match_ms: the walker launches of the call), the three calls ALTERNATING round by round, medians of R rounds after one
warm-up round:
  (a) bsg_match_rows_range with FieldRange("timestamp", lo, hi) selecting about 1 % of the rows;
  (b) bsg_match_rows_tok with Field("timestamp"): the same walker without the consumer;
  (c) bsg_match_rows_regex with FieldRegex("timestamp", "^17000[0-9]+$"): the cheapest consumer the project ships on the same leaf.
The bar: (a) <= (c) under both specs, with a margin equal to the spread (max - min) the R rounds of (c) themselves show — the number
lane does strictly less per byte than a DFA step with an LDS read.  (a) / (b) is recorded without a bar: the cost of the feature.
Writes profiles/match_range_lab.txt and exits 1 when the bar is missed.

    python tools/match_range_lab.py [n_rows] [rounds]
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
TRIGRAM = Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
lo = synth.TS_BASE + n_rows // 2
hi = lo + n_rows // 100 - 1
lines = ["# python tools/match_range_lab.py %d %d — synth log rows; ms = bsg_last_match_ms, the calls alternating, median of %d rounds (min .. max)"
         % (n_rows, rounds, rounds), "rows %d, %.1f MB of row bytes; FieldRange(timestamp, %d, %d)" % (n_rows, int(off[-1]) / 1e6, lo, hi)]
ok = True
with Context((0,)) as ctx:
    for name, spec in (("default", None), ("trigram", TRIGRAM)):
        rng = Q.CompiledRangeQuery(None, Q.FieldRange("timestamp", lo, hi))
        fld = Q.CompiledMatcher(Q.Field("timestamp"))
        rgx = Q.CompiledRowQuery(None, Q.FieldRegex("timestamp", "^17000[0-9]+$"))
        calls = [("a", lambda: ctx.match_rows_range((blob, off), rng, spec)), ("b", lambda: ctx.match_rows((blob, off), fld, tokenizer=spec)),
                 ("c", lambda: ctx.match_rows_regex((blob, off), rgx, tokenizer=spec))]
        ms = {k: [] for k, _ in calls}
        out = {}
        for r in range(rounds + 1):
            for k, fn in calls:
                out[k] = fn()
                if r:
                    ms[k].append(ctx.last_match_ms())
        assert all(len(fb) == 0 for _, fb in out.values())
        assert int(out["a"][0].sum()) == hi - lo + 1 and out["b"][0].all()
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(ms["c"]) - min(ms["c"])
        passed = med["a"] <= med["c"] + spread
        ok = ok and passed
        for k, what in (("a", "bsg_match_rows_range FieldRange(timestamp)"), ("b", "bsg_match_rows_tok Field(timestamp)"), ("c", "bsg_match_rows_regex ^17000[0-9]+$")):
            lines.append("%-8s (%s) %-44s %8.3f ms (%.3f .. %.3f), %d rows" % (name, k, what, med[k], min(ms[k]), max(ms[k]), int(out[k][0].sum())))
        lines.append("%-8s (a) / (b) = %.3f   (a) <= (c) + spread of (c): %.3f <= %.3f + %.3f: %s"
                     % (name, med["a"] / med["b"], med["a"], med["c"], spread, "met" if passed else "MISSED"))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "match_range_lab.txt"), "w") as f:
    f.write(text)
sys.exit(0 if ok else 1)
