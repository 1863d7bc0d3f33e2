"""One bsg_match_rows_many call against Q bsg_match_rows calls: synth log rows in page-locked memory, Q in {1, 8, 64} queries of the
bench's C2 shape (And of three FieldToken drawn from the 29 distinct level / service / nested.region terms).  Per Q: device time
(bsg_last_match_ms) and wall time of the many-call and of the Q single calls, medians over R runs with the run-to-run spread
(min .. max).  --singles-only measures the single calls alone, so that the same script runs against a library built from
another commit (--lib PATH) on the same box.

    python tools/match_many_lab.py [n_rows] [repeats] [--singles-only] [--lib PATH]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bloomsearch_amd import _lib  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    args.remove(sys.argv[sys.argv.index("--lib") + 1])
singles_only = "--singles-only" in sys.argv
from bloomsearch_amd import query as Q, synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402

n_rows = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 7
rows = synth.rows_json(0, n_rows)
off = np.zeros(n_rows + 1, dtype=np.uint64)
off[1:] = np.cumsum([len(r) for r in rows])
n_bytes = int(off[-1])
d = synth.draws(0, 64)
exprs = [Q.And(Q.FieldToken("level", synth.LEVELS[d["level"][i]]), Q.FieldToken("service", synth.SERVICES[d["service"][i]]),
               Q.FieldToken("nested.region", "region-%d" % int(d["region"][i]))) for i in range(64)]
print("library %s\nrows %d, %.1f MB of row bytes in page-locked memory, %d runs per figure: median (min .. max)" % (_lib.LIB_PATH, n_rows, n_bytes / 1e6, reps))


def fmt(v):
    return "%9.2f (%8.2f .. %8.2f)" % (float(np.median(v)), min(v), max(v))


with Context((0,)) as ctx:
    blob = ctx.pinned_array(n_bytes)
    blob[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
    del rows
    ctx.match_rows((blob, off), Q.CompiledMatcher(exprs[0]))                      # warm: module load, scratch, lower table
    base = None
    for nq in (1, 8, 64):
        matchers = [Q.CompiledMatcher(e) for e in exprs[:nq]]
        s_dev, s_wall = [], []
        for _ in range(reps):
            dev, t0 = 0.0, time.perf_counter()
            for m in matchers:
                hits, fb = ctx.match_rows((blob, off), m)
                dev += ctx.last_match_ms()
            s_wall.append((time.perf_counter() - t0) * 1e3)
            s_dev.append(dev)
        print("Q=%2d  %2d x bsg_match_rows      device ms %s   wall ms %s" % (nq, nq, fmt(s_dev), fmt(s_wall)))
        if singles_only:
            continue
        batch = Q.CompiledMatcherBatch(exprs[:nq])
        planes, fb = ctx.match_rows_many((blob, off), batch)
        assert len(fb) == 0 and np.array_equal(planes[nq - 1], hits)
        m_dev, m_wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.match_rows_many((blob, off), batch)
            m_wall.append((time.perf_counter() - t0) * 1e3)
            m_dev.append(ctx.last_match_ms())
        base = base or float(np.median(m_dev))
        print("Q=%2d   1 x bsg_match_rows_many device ms %s   wall ms %s   %d conditions" % (nq, fmt(m_dev), fmt(m_wall), len(batch.kinds)))
        print("Q=%2d  many / singles: device %.3f, wall %.3f; many-kernel vs its Q=1: %.3f; %.1f M rows/s, %.1f GB/s of row bytes on the device"
              % (nq, np.median(m_dev) / np.median(s_dev), np.median(m_wall) / np.median(s_wall), np.median(m_dev) / base,
                 n_rows / np.median(m_dev) / 1e3, n_bytes / np.median(m_dev) / 1e6))
    ctx.pinned_free(blob)
