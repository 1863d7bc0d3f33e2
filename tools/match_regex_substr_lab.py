"""FieldRegex and substring conditions in one device walk (bsg_match_rows_regex_substr) against the two walks it replaces, on the rows
tools/match_substr_lab.py uses: synth log rows, under the default and the trigram spec.  Two shapes: one regex condition plus one
needle; 4 regex conditions plus 8 needles.  Per shape three calls over the same rows:
  - the combined call, program And(Or of the regex conditions, Or of the needles);
  - bsg_match_rows_regex (bsg_match_rows_tok under a spec) with the regex conditions alone;
  - bsg_match_rows_substr with the needles alone.
Kernel time = bsg_last_match_ms (the walker launches of the call); the three calls alternate, R rounds after one warm-up round, the
median of each is reported, and combined / (regex + substr) is the figure: below 1 the one walk is cheaper than the two.

    python tools/match_regex_substr_lab.py [n_rows] [rounds]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SPECS = {"default": None, "trigram": Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)}
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
print("# python tools/match_regex_substr_lab.py %d %d — synth log rows; ms = bsg_last_match_ms, the three calls alternating, median of %d rounds"
      % (n_rows, rounds, rounds))
print("rows %d, %.1f MB of row bytes" % (n_rows, int(off[-1]) / 1e6))

REGEXES = [Q.FieldRegex("message", "timeout|cache"), Q.FieldRegex("service", "^(auth|pay)"), Q.FieldRegex("nested.region", "region-[37]$"),
           Q.FieldRegex("level", "(?i)error")]
NEEDLES = ["ion time", "che miss", "y reques", "eout", "pstrea", "ed cache", "atenc", "ss shard"]
SHAPES = [("1 regex + 1 needle", REGEXES[:1], NEEDLES[:1]), ("4 regex + 8 needles", REGEXES, NEEDLES)]

with Context((0,)) as ctx:
    for spec_name, spec in SPECS.items():
        for shape, regexes, needles in SHAPES:
            rx, sx = Q.RegexOr(*regexes), Q.SubstringOr(*[Q.Substring(n) for n in needles])
            calls = {
                "combined": lambda: ctx.match_rows_regex_substr((blob, off), Q.CompiledRowSubstringQuery(None, rx, sx), spec),
                "regex": lambda: ctx.match_rows_regex((blob, off), Q.CompiledRowQuery(None, rx), spec),
                "substr": lambda: ctx.match_rows_substr((blob, off), Q.CompiledSubstringQuery(None, sx), spec),
            }
            ms = {k: [] for k in calls}
            out = {}
            for r in range(rounds + 1):
                for k, fn in calls.items():
                    out[k] = fn()
                    if r:
                        ms[k].append(ctx.last_match_ms())
            assert all(len(fb) == 0 for _, fb in out.values())
            assert np.array_equal(out["combined"][0], out["regex"][0] & out["substr"][0]), "the one walk and the two walks disagree"
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print("%-7s %-19s: combined %7.3f ms | bsg_match_rows_regex %7.3f ms + bsg_match_rows_substr %7.3f ms = %7.3f ms | combined / sum %.3f, "
                  "combined / dearer %.3f | %d rows match" % (spec_name, shape, med["combined"], med["regex"], med["substr"], med["regex"] + med["substr"],
                                                               med["combined"] / (med["regex"] + med["substr"]), med["combined"] / max(med["regex"], med["substr"]),
                                                               int(out["combined"][0].sum())))
