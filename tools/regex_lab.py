"""Device FieldRegex matching (bsg_match_rows_regex) on synth log rows: device ms (bsg_last_match_ms, the best of R calls),
rows/s and GB/s of row bytes for the QueryRegex shape of the reference's bench (FieldToken("level","error") +
FieldRegex("message","timeout|cache")), ^QuoteMeta(text)$, [0-9]{3}-[0-9]{4} and (?i)error; the same rows under the plain
Field / Token matcher (bsg_match_rows); the per-call compile cost of the patterns; and the host mirror's std::regex path
(bsh_match_row_regex, one row per call) on a slice of the rows.

    python tools/regex_lab.py [n_rows] [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import host as Hst, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402

n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
n_bytes = int(off[-1])
print("rows %d, %.1f MB of row bytes" % (n_rows, n_bytes / 1e6))

shapes = [
    ("plain FieldToken(level,error)", "plain", Q.FieldToken("level", "error"), None),
    ("plain And(FieldToken(level,error), Token(cache))", "plain", Q.And(Q.FieldToken("level", "error"), Q.Token("cache")), None),
    ("QueryRegex: FieldToken(level,error) + FieldRegex(message, timeout|cache)", "regex", Q.FieldToken("level", "error"),
     Q.FieldRegex("message", "timeout|cache")),
    ("FieldRegex(message, timeout|cache) alone", "regex", None, Q.FieldRegex("message", "timeout|cache")),
    ("FieldRegex(service, ^billing$) [^QuoteMeta(text)$]", "regex", None, Q.FieldRegex("service", "^billing$")),
    ("FieldRegex(message, [0-9]{3}-[0-9]{4})", "regex", None, Q.FieldRegex("message", "[0-9]{3}-[0-9]{4}")),
    ("FieldRegex(message, (?i)error)", "regex", None, Q.FieldRegex("message", "(?i)error")),
]
with Context((0,)) as ctx:
    for name, kind, bloom, rx in shapes:
        m = Q.CompiledMatcher(bloom) if kind == "plain" else Q.CompiledRowQuery(bloom, rx)
        fn = ctx.match_rows if kind == "plain" else ctx.match_rows_regex
        fn((blob, off), m)                                  # warm
        best, wall = 1e9, 1e9
        for _ in range(reps):
            t0 = time.perf_counter()
            hits, fb = fn((blob, off), m)
            wall = min(wall, time.perf_counter() - t0)
            best = min(best, ctx.last_match_ms())
        print("%-75s device %8.3f ms  %7.1f M rows/s  %6.1f GB/s   (call %.1f ms, %d hits, %d fallback)"
              % (name, best, n_rows / best / 1e3, n_bytes / best / 1e6, wall * 1e3, int(hits.sum()), len(fb)))
    # what compiling the patterns costs per call: a call over one 10 000-row block (a typical surviving block) with and without
    # the regex condition's compile
    small = rows[:10000]
    for name, rx in (("timeout|cache", Q.FieldRegex("message", "timeout|cache")), ("(?i)error", Q.FieldRegex("message", "(?i)error")),
                     ("[0-9]{3}-[0-9]{4}", Q.FieldRegex("message", "[0-9]{3}-[0-9]{4}"))):
        m = Q.CompiledRowQuery(None, rx)
        ctx.match_rows_regex(small, m)
        t = []
        for _ in range(20):
            t0 = time.perf_counter(); ctx.match_rows_regex(small, m); t.append(time.perf_counter() - t0)
        c = []
        for _ in range(200):
            t0 = time.perf_counter(); Hst.regex_match(rx["Condition"]["Pattern"], ""); c.append(time.perf_counter() - t0)
        print("10 000-row call with %-20s %.3f ms; compile + one empty run on the host %.4f ms (%.1f %%)"
              % (name, np.median(t) * 1e3, np.median(c) * 1e3, 100 * np.median(c) / np.median(t)))

# the host mirror's std::regex row test, one row per call
n_host = min(n_rows, 20000)
for name, rx in (("timeout|cache", Q.FieldRegex("message", "timeout|cache")), ("(?i)error", Q.FieldRegex("message", "(?i)error"))):
    t0 = time.perf_counter()
    for r in rows[:n_host]:
        Hst.match_row_regex(rx, r)
    dt = time.perf_counter() - t0
    hb = int(off[n_host])
    print("host mirror std::regex FieldRegex(message, %-14s %8.1f ms per %d rows  %7.3f M rows/s  %6.3f GB/s"
          % (name + ")", dt * 1e3, n_host, n_host / dt / 1e6, hb / dt / 1e9))
