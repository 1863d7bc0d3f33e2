"""Lab: the program evaluator by itself at the headline's shape — the bench's C2 arena (1 000 blocks x 10 000 rows, fpr 0.001) and
batch (4 096 three-term Ands, 29 distinct terms), 16 rotating replicas, survivors left on the device.

    python tools/eval_rows_lab.py eval [rounds [arenas,..]]
        the evaluation dispatch alone (k_eval_programs / _ext behind one plain gather dispatch, lab key 27 = 1) at 20, 67 and 200
        arenas per call: the dispatch's own timestamps (BSG_PROBE_TIMED), median (min .. max) of `rounds` calls (default 24)
    python tools/eval_rows_lab.py call [rounds [arenas,..]]
        the whole call under the planner (key 27 = 0): summed kernel time of a timed call and the wall time of an untimed one

One process runs ONE variant; a sitting runs the variants in turn, process after process:
    BSG_LAB_LIB=path            another build of the library: the parent's, or this tree's with
                                BSG_EXTRA_CXXFLAGS=-DBSG_LAB_EVAL_NO_STORES    (survivor stores compiled out)
                                BSG_EXTRA_CXXFLAGS=-DBSG_LAB_EVAL_NO_VERDICTS  (verdict loads and transposes compiled out, stores kept)
                                BSG_EXTRA_CXXFLAGS=-DBSG_EVAL_ROW_SPAN=16      (spans of 16 groups: whole 128-byte lines per workgroup)
    BSG_LAB_EVAL_ROWS=0         eval_role_all where the row spans would run (read once per process by the library)
BSG_LAB_CACHE=dir keeps the built arena between runs.  The numbers on record: profiles/eval_rows_lab.txt.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from probe_gather_lab import batch_of, c2_arenas, bench, Context, _lib, synth

ARENAS = (20, 67, 200)


def med(v):
    return "%7.1f (%7.1f .. %7.1f)" % (float(np.median(v)), min(v), max(v))


def one_call(ctx, arenas, bid, n, step, timed):
    ids = np.ascontiguousarray([arenas[(step + j) % len(arenas)] for j in range(n)], dtype=np.uint64)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.probe_many(ids, bid, _lib.PROBE_ASYNC | (_lib.PROBE_TIMED if timed else 0))
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6
    return ctx.timing_read(reset=True) if timed else wall


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "eval"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    arenas_list = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else ARENAS
    if mode not in ("eval", "call") or rounds < 16:
        sys.exit(__doc__)
    print("library %s  BSG_LAB_EVAL_ROWS=%s" % (_lib.LIB_PATH, os.environ.get("BSG_LAB_EVAL_ROWS", "(unset)")), flush=True)
    bench.start_pool(16)
    ctx = Context((0,))
    ctx.set_lab(3, 0)
    ctx.set_timed_stride(1)
    arenas, B = c2_arenas(ctx)
    bid, nq, nt = batch_of(ctx, synth.make_queries(4096, "c2", seed=1234))
    print("C2: %d queries, %d distinct terms, arenas of %d blocks, %d replicas; us, median (min .. max) of %d calls" % (nq, nt, B, len(arenas), rounds))
    ctx.set_lab(27, 1 if mode == "eval" else 0)
    step, warm = 0, 3
    res = {n: ([], [], []) for n in arenas_list}
    for i in range(warm + rounds):
        for n in arenas_list:                                 # the arena counts in turn, call by call
            tm = one_call(ctx, arenas, bid, n, step, True)
            step += n
            assert tm.n_probe_arenas + tm.n_fused_arenas == n and tm.n_eval == 1, (n, tm.n_probe_arenas, tm.n_fused_arenas, tm.n_eval)
            wall = one_call(ctx, arenas, bid, n, step, False)
            step += n
            if i >= warm:
                res[n][0].append(tm.ms_eval_kernel * 1e3)
                res[n][1].append((tm.ms_terms_kernel + tm.ms_fused_kernel + tm.ms_eval_kernel) * 1e3)
                res[n][2].append(wall)
    for n in arenas_list:
        e, k, w = res[n]
        print("%3d arenas  %s dispatch %s   per arena %.3f   kernels %s   wall %s"
              % (n, "evaluation" if mode == "eval" else "last evaluation", med(e), float(np.median(e)) / n, med(k), med(w)), flush=True)
    ctx.set_lab(27, 0)
    bench.stop_pool()


if __name__ == "__main__":
    main()
