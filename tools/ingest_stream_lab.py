"""Streaming device ingest against the one-shot call on the same rows (synth log rows over 16 sets, one parent):

  leg (a)  one bsg_ingest_rows call on the rows grouped by set, then bsg_ingest_finish
  leg (b)  bsg_ingest_open, then B bsg_ingest_append_rows calls of the same rows INTERLEAVED over the sets (row i of the
           stream belongs to set i % 16), for B in {1, 16, 256}, then bsg_ingest_finish

Printed per leg: the wall time of the finish-side work (what a flush pays: for (a) the ingest call AND the finish, for (b) the
finish alone — its appends ran when the batches arrived), the summed ms_walk (walker dispatch time over all launches,
bsg_ingest_stats), the total wall of all calls, and table_grows.  Walls are host clocks around calls that return synchronised.
The legs alternate inside one process, one untimed warm-up round first, R timed rounds; every figure is the median of the
rounds, the spread (min .. max) of the total wall beside it.  Both legs must count the same distinct entries, or the tool fails.

--lib PATH runs the same script against a library built from another commit on the same box.

    python tools/ingest_stream_lab.py [n_rows] [rounds] [--lib PATH]
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
from bloomsearch_amd import synth  # noqa: E402
from bloomsearch_amd.gpu import Context  # noqa: E402

N_SETS = 16
n_rows = int(args[0]) if len(args) > 0 else 1_000_000
rounds = int(args[1]) if len(args) > 1 else 5
per_set = n_rows // N_SETS
n_rows = per_set * N_SETS


def pack(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.frombuffer(b"".join(rows), dtype=np.uint8), off


row_sets = [synth.rows_json(s * per_set, per_set) for s in range(N_SETS)]
grouped = pack([r for rs in row_sets for r in rs])
first = np.arange(N_SETS + 1, dtype=np.uint32) * per_set
stream_rows = [row_sets[i % N_SETS][i // N_SETS] for i in range(n_rows)]      # arrival order: the sets interleaved row by row
set_of_row = (np.arange(n_rows) % N_SETS).astype(np.uint32)
parents = [0] * N_SETS


def batches(B):
    cuts = [n_rows * b // B for b in range(B + 1)]
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        blob, off = pack(stream_rows[lo:hi])
        out.append(((blob, off), set_of_row[lo:hi]))
    return out


def leg_one_shot(ctx):
    t0 = time.perf_counter()
    ing = ctx.ingest_rows(grouped, first, parents, 1, flags=_lib.INGEST_TRUSTED_JSON)
    assert len(ctx.ingest_fallback_rows(ing)) == 0
    counts, status = ctx.ingest_finish(ing, N_SETS + 1)
    t1 = time.perf_counter()
    st = ctx.ingest_stats(ing)
    ctx.ingest_free(ing)
    assert not status.any()
    return dict(flush_ms=(t1 - t0) * 1e3, walk_ms=st.ms_walk, total_ms=(t1 - t0) * 1e3, grows=st.table_grows), counts


def leg_stream(ctx, bs):
    t0 = time.perf_counter()
    ing = ctx.ingest_open(N_SETS, parents, 1, flags=_lib.INGEST_TRUSTED_JSON)
    for rows, sor in bs:
        assert len(ctx.ingest_append_rows(ing, rows, sor)) == 0
    t1 = time.perf_counter()
    counts, status = ctx.ingest_finish(ing, N_SETS + 1)
    t2 = time.perf_counter()
    st = ctx.ingest_stats(ing)
    ctx.ingest_free(ing)
    assert not status.any()
    return dict(flush_ms=(t2 - t1) * 1e3, walk_ms=st.ms_walk, total_ms=(t2 - t0) * 1e3, grows=st.table_grows), counts


def main():
    print("# library %s" % _lib.LIB_PATH)
    print("# python tools/ingest_stream_lab.py %d %d — synth log rows, %d sets of %d rows, one parent, BSG_INGEST_TRUSTED_JSON;\n"
          "# %.1f MB of row bytes; legs alternate in one process, 1 warm-up round + %d timed rounds, medians (total wall: min .. max)"
          % (n_rows, rounds, N_SETS, per_set, int(grouped[1][-1]) / 1e6, rounds))
    legs = [("(a) one bsg_ingest_rows call, grouped", None)] + [("(b) open + %3d appends, interleaved" % B, batches(B)) for B in (1, 16, 256)]
    res = {name: [] for name, _ in legs}
    with Context((0,)) as ctx:
        want = None
        for rnd in range(rounds + 1):
            for name, bs in legs:
                r, counts = leg_one_shot(ctx) if bs is None else leg_stream(ctx, bs)
                if want is None:
                    want = counts
                assert np.array_equal(counts, want), "%s counts differently" % name
                if rnd:
                    res[name].append(r)
    print("%-42s %14s %14s %26s %12s" % ("leg", "flush-side ms", "sum ms_walk", "total wall ms (min..max)", "table_grows"))
    for name, _ in legs:
        rs = res[name]
        med = lambda k: float(np.median([r[k] for r in rs]))   # noqa: E731
        tot = [r["total_ms"] for r in rs]
        print("%-42s %14.2f %14.2f %12.2f (%.2f..%.2f) %12d" % (name, med("flush_ms"), med("walk_ms"), med("total_ms"), min(tot), max(tot), rs[0]["grows"]))


if __name__ == "__main__":
    main()
