"""Range, regex and substring conditions in one device walk (bsg_match_rows_regex_substr_range) against the TWO calls a C-ABI caller
makes for such a query without it, each with its own side of the table over the same rows:
  - bsg_match_rows_range with the range conditions;
  - bsg_match_rows_regex_substr with the text conditions (bsg_match_rows_substr / bsg_match_rows_regex where one text side is empty).
Synth log rows under the default and the trigram spec, three settings: 1 range + 1 needle; 1 range + 1 regex + 1 needle; 16 ranges +
4 regex + 8 needles.  The program is And(Or of the ranges, [Or of the regex conditions,] Or of the needles), so the one call's bits are
the AND of the two calls' bits (asserted).  Kernel time = bsg_last_match_ms (the walker launches of the call); the calls alternate, R
rounds after one warm-up round, medians.
The bar: the one walk below the SUM of the two it replaces, by more than the spread (max - min over the rounds) of that sum: MET when
one + spread < sum, MISSED otherwise.  one / dearer is reported beside it.  Every line goes to profiles/match_range_text_lab.txt.

    python tools/match_range_text_lab.py [n_rows] [rounds] [out_file]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "match_range_text_lab.txt")
SPECS = {"default": None, "trigram": Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)}
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
T0 = 1700000000                                                  # synth: row i has timestamp T0 + i
lines = ["# python tools/match_range_text_lab.py %d %d — synth log rows; ms = bsg_last_match_ms, the calls alternating, median of %d rounds"
         % (n_rows, rounds, rounds), "rows %d, %.1f MB of row bytes" % (n_rows, int(off[-1]) / 1e6)]
print("\n".join(lines))

REGEXES = [Q.FieldRegex("message", "timeout|cache"), Q.FieldRegex("service", "^(auth|pay)"), Q.FieldRegex("nested.region", "region-[37]$"),
           Q.FieldRegex("level", "(?i)error")]
NEEDLES = ["ion time", "che miss", "y reques", "eout", "pstrea", "ed cache", "atenc", "ss shard"]
half = n_rows // 2
ONE_RANGE = [Q.FieldRange("timestamp", T0 + half // 2, T0 + half // 2 + half)]           # a window over half of the rows
# 8 windows of timestamp (together about a quarter of the rows) and 8 of user_id
MANY_RANGES = [Q.FieldRange("timestamp", T0 + k * (n_rows // 8), T0 + k * (n_rows // 8) + n_rows // 32) for k in range(8)] + \
              [Q.FieldRange("user_id", 10000 * k, 10000 * k + 2500, hi_open=True) for k in range(8)]
SETTINGS = [("1 range + 1 needle", ONE_RANGE, [], NEEDLES[:1]), ("1 range + 1 regex + 1 needle", ONE_RANGE, REGEXES[:1], NEEDLES[:1]),
            ("16 ranges + 4 regex + 8 needles", MANY_RANGES, REGEXES, NEEDLES)]

with Context((0,)) as ctx:
    for spec_name, spec in SPECS.items():
        for setting, ranges, regexes, needles in SETTINGS:
            rg, sx = Q.RangeOr(*ranges), Q.SubstringOr(*[Q.Substring(n) for n in needles])
            rx = Q.RegexOr(*regexes) if regexes else None
            if regexes:
                text_name, text = "bsg_match_rows_regex_substr", lambda: ctx.match_rows_regex_substr((blob, off), Q.CompiledRowSubstringQuery(None, rx, sx), spec)
            else:
                text_name, text = "bsg_match_rows_substr", lambda: ctx.match_rows_substr((blob, off), Q.CompiledSubstringQuery(None, sx), spec)
            calls = {
                "one": lambda: ctx.match_rows_regex_substr_range((blob, off), Q.CompiledRowTextRangeQuery(None, rx, sx, rg), spec),
                "range": lambda: ctx.match_rows_range((blob, off), Q.CompiledRangeQuery(None, rg), spec),
                "text": text,
            }
            ms = {k: [] for k in calls}
            out = {}
            for r in range(rounds + 1):
                for k, fn in calls.items():
                    out[k] = fn()
                    if r:
                        ms[k].append(ctx.last_match_ms())
            assert all(len(fb) == 0 for _, fb in out.values())
            assert np.array_equal(out["one"][0], out["range"][0] & out["text"][0]), "the one walk and the two walks disagree"
            med = {k: float(np.median(v)) for k, v in ms.items()}
            sums = [a + b for a, b in zip(ms["range"], ms["text"])]
            total, spread = med["range"] + med["text"], max(sums) - min(sums)
            line = ("%-7s %-31s: one walk %7.3f ms (min %.3f max %.3f) | bsg_match_rows_range %7.3f ms + %s %7.3f ms = %7.3f ms (spread of the sum over the rounds "
                    "%.3f ms) | one / sum %.3f, one / dearer %.3f | %s | %d rows match"
                    % (spec_name, setting, med["one"], min(ms["one"]), max(ms["one"]), med["range"], text_name, med["text"], total, spread, med["one"] / total,
                       med["one"] / max(med["range"], med["text"]), "MET" if med["one"] + spread < total else "MISSED", int(out["one"][0].sum())))
            print(line, flush=True)
            lines.append(line)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
