"""bsg_match_rows_wide_hist against what a histogram of hits costs without it: synth log rows in page-locked memory, 16 sets, a batch of
token, range and substring queries listed on every set, at a sparse and at a dense match rate, bucketed by `timestamp` into B = 60 and
B = 1 024 buckets.  Before anything is timed the counts are compared, slot for slot, with the counts derived from every row of the
parent's row lists.
  (1) the walk plus the evaluation inside the new call (bsg_last_match_ms) | bsg_match_rows_wide_regex_substr_range on the same batch
      (bsg_last_match_ms): the same kernels, expected equal within the session's own spread
  (2) k_bucket_rows (bsg_last_hist_ms of a call whose one pair per set matches no row: the scanner plus a counting pass over all-zero
      words) | the one-field k_minmax_rows over the same rows (bsg_last_minmax_ms of bsg_ingest_rows_minmax): the same bytes, the same scanner
  (3) the new call's wall time | bsg_match_rows_wide_regex_substr_range_rows' wall time plus the host time to bucket its listed rows with
      bsh_hist_row (timed over at most SAMPLE listed rows and scaled to all of them; the loop is Python's, one ctypes call per row, so
      the figure holds the interpreter's cost per call beside the parse: no native loop is measured here)
The sides alternate within a round, R rounds after one warm-up round; per figure the median (min .. max).  MET / NOT MET is stated per
comparison from these figures alone: (1) |difference of the medians| <= the larger of the two sides' (max - min); (2) the scanner's
median <= the yardstick's median plus the yardstick's (max - min); (3) the new call's median wall <= the other side's.

    python tools/match_hist_lab.py [n_rows] [rounds] [out_file]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bloomsearch_amd import _lib, host, query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context, pair_rows_list  # noqa: E402

args = sys.argv[1:]
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "match_hist_lab.txt")
N_SETS, SAMPLE, FIELD = 16, 100_000, "timestamp"
T0 = synth.TS_BASE                                               # synth: row i has timestamp T0 + i
BATCHES = {
    "sparse": [(Q.FieldToken("level", synth.LEVELS[0]), None, None, Q.FieldRange("user_id", 100, 140)), (None, None, None, Q.FieldRange("timestamp", T0 + 1000, T0 + 3000)),
               (None, None, Q.Substring("che miss"), Q.FieldRange("user_id", 0, 2000)), (Q.Token(synth.WORDS[0]), None, Q.FieldSubstring("message", "pstrea"), None)],
    "dense": [(Q.FieldToken("level", synth.LEVELS[0]), None, None, None), (None, None, None, Q.FieldRange("timestamp", T0, T0 + n_rows // 2)),
              (None, None, Q.Substring("e"), None), (None, None, None, None)],
}


def fmt(v):
    return "%9.3f (%9.3f .. %9.3f)" % (float(np.median(v)), min(v), max(v))


def spread(v):
    return max(v) - min(v)


rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
first = np.array([s * n_rows // N_SETS for s in range(N_SETS + 1)], dtype=np.uint32)
lines = ["# python tools/match_hist_lab.py %d %d" % (n_rows, reps),
         "rows %d, %.1f MB of row bytes in page-locked memory, %d sets; every query listed on every set; the bucket field is `%s`" % (n_rows, n_bytes / 1e6, N_SETS, FIELD),
         "ms: median (min .. max) of %d alternating rounds after one warm-up round" % reps]
print("\n".join(lines), flush=True)
verdicts = {1: [], 2: [], 3: []}
with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    data = (blob, off)
    for B in (60, 1024):
        origin, width = T0, n_rows // B + 1
        never = Q.CompiledWideTextRangeBatch([(None, None, None, Q.FieldRange("user_id", 5, 4))])
        one_off, one_sq = np.arange(N_SETS + 1, dtype=np.uint32), np.zeros(N_SETS, dtype=np.uint32)
        for rate, quads in BATCHES.items():
            batch = Q.CompiledWideTextRangeBatch(quads)
            nq = len(quads)
            sq_off = np.arange(N_SETS + 1, dtype=np.uint32) * nq
            sq = np.tile(np.arange(nq, dtype=np.uint32), N_SETS)

            def hist():
                t = time.perf_counter()
                counts, fb = ctx.match_rows_wide_hist(data, batch, FIELD, origin, width, B, first, sq_off, sq)
                return counts, fb, ctx.last_match_ms(), ctx.last_hist_ms(), (time.perf_counter() - t) * 1e3

            def listed():
                t = time.perf_counter()
                hdr, pair_off, payload, fb = ctx.match_rows_wide_regex_substr_range_rows(data, batch, first, sq_off, sq)
                return hdr, pair_off, payload, fb, ctx.last_match_ms(), (time.perf_counter() - t) * 1e3

            def bucket(hdr, pair_off, payload, sample=True):
                """the host's side of today's route: every listed row parsed for its slot (sample: at most SAMPLE of them, the time
                scaled) -> (counts, ms, listed rows, stride)"""
                counts = np.zeros((len(hdr), B + 3), dtype=np.uint32)
                todo = []
                for s in range(N_SETS):
                    for p in range(int(sq_off[s]), int(sq_off[s + 1])):
                        ids = pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], int(first[s + 1]) - int(first[s]))
                        todo.append((p, ids + int(first[s])))
                total = sum(len(ids) for _, ids in todo)
                stride = max(1, total // SAMPLE) if sample else 1
                t, done = time.perf_counter(), 0
                for p, ids in todo:
                    for r in ids[::stride]:
                        counts[p, host.hist_row(rows[int(r)], FIELD, origin, width, B)] += 1
                        done += 1
                ms = (time.perf_counter() - t) * 1e3
                return counts, (ms * total / done if done else 0.0), total, stride

            # the same counts first (this is also the warm-up round)
            counts, fb, _, _, _ = hist()
            hdr, pair_off, payload, rfb, _, _ = listed()
            assert list(fb) == list(rfb) == []
            want, _, total, _ = bucket(hdr, pair_off, payload, sample=False)      # every listed row, once: the counts slot for slot
            assert np.array_equal(counts, want), (B, rate)
            assert int(counts.sum()) == total, (B, rate, int(counts.sum()), total)
            stride = max(1, total // SAMPLE)
            ctx.match_rows_wide_regex_substr_range(data, batch, first, sq_off, sq)
            fig = {k: [] for k in ("hist_match", "hist_hist", "hist_wall", "words_match", "rows_match", "rows_wall", "bucket", "scanner", "minmax")}
            for _ in range(reps):
                _, _, m, h, w = hist()
                fig["hist_match"].append(m); fig["hist_hist"].append(h); fig["hist_wall"].append(w)
                ctx.match_rows_wide_regex_substr_range(data, batch, first, sq_off, sq)
                fig["words_match"].append(ctx.last_match_ms())
                hdr, pair_off, payload, _, m, w = listed()
                fig["rows_match"].append(m); fig["rows_wall"].append(w)
                fig["bucket"].append(bucket(hdr, pair_off, payload)[1])
                ctx.match_rows_wide_hist(data, never, FIELD, origin, width, B, first, one_off, one_sq)
                fig["scanner"].append(ctx.last_hist_ms())
                iid = ctx.ingest_rows(data, first, minmax_fields=[FIELD])
                fig["minmax"].append(ctx.last_minmax_ms())
                ctx.ingest_free(iid)
            med = {k: float(np.median(v)) for k, v in fig.items()}
            ok1 = abs(med["hist_match"] - med["words_match"]) <= max(spread(fig["hist_match"]), spread(fig["words_match"]))
            ok2 = med["scanner"] <= med["minmax"] + spread(fig["minmax"])
            other = [a + b for a, b in zip(fig["rows_wall"], fig["bucket"])]
            ok3 = med["hist_wall"] <= float(np.median(other))
            for k, ok in ((1, ok1), (2, ok2), (3, ok3)):
                verdicts[k].append(ok)
            head = "B=%4d %-6s %d queries x %d sets, %9d listed rows" % (B, rate, nq, N_SETS, total)
            out = [
                "%s | new call: bsg_last_match_ms %s, bsg_last_hist_ms %s, wall %s" % (head, fmt(fig["hist_match"]), fmt(fig["hist_hist"]), fmt(fig["hist_wall"])),
                "%s | (1) walk + evaluation in the new call %s | bsg_match_rows_wide_regex_substr_range %s | %s" %
                (head, fmt(fig["hist_match"]), fmt(fig["words_match"]), "MET" if ok1 else "NOT MET"),
                "%s | (2) k_bucket_rows (+ a counting pass over zero words) %s | one-field k_minmax_rows %s | %s" % (head, fmt(fig["scanner"]), fmt(fig["minmax"]), "MET" if ok2 else "NOT MET"),
                "%s | (3) new call wall %s | _rows call: kernels %s, wall %s + host bucketing (every %d-th listed row timed, scaled) %s = %s | %s" %
                (head, fmt(fig["hist_wall"]), fmt(fig["rows_match"]), fmt(fig["rows_wall"]), stride, fmt(fig["bucket"]), fmt(other), "MET" if ok3 else "NOT MET"),
            ]
            for line in out:
                print(line, flush=True)
            lines += out
    ctx.pinned_free(blob)
summary = ["(%d) %s" % (k, "MET" if all(v) else "NOT MET (in %d of %d configurations)" % (len(v) - sum(v), len(v))) for k, v in verdicts.items()]
lines.append("overall: " + "; ".join(summary))
print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
