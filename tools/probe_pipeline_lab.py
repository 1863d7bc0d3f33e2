"""Lab: the chunked gather (bsg_set_lab key 27: k_probe_gather on chunk 0, k_gather_fused = gather chunk i + evaluate chunk i - 1,
k_eval_programs on the last chunk) against the two plain dispatches, at the headline's shape: the bench's C2 arena (1 000 blocks x
10 000 rows, fpr 0.001) and batch (4 096 three-term Ands, 29 distinct terms), 16 rotating replicas, survivors left on the device.

    python tools/probe_pipeline_lab.py grid [rounds [arenas,.. [chunks,..]]]
                                                          20 / 50 / 100 / 200 arenas per call x 1 / 2 / 3 / 4 / 6 chunks, the evaluation workgroups in front of
                                                          k_gather_fused's grid or spread through it, equal chunks and a last chunk of half a share: kernel time (the dispatches' own timestamps, summed) and
                                                          call wall time (enqueue .. stream drained, no timestamps), the configurations in turn
    python tools/probe_pipeline_lab.py default [rounds]   key 27 = 0 (the planner) against key 27 = 1 at the same arena counts, wall time

BSG_LAB_LIB=path loads another build of the library; one that does not know key 27 runs the one-chunk rows only (the parent's figures).
BSG_LAB_CACHE=dir keeps the built arena between runs.  The numbers on record: profiles/probe_pipeline_lab.txt.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from probe_gather_lab import batch_of, c2_arenas, bench, Context, _lib, synth

ARENAS = (20, 50, 100, 200)
CHUNKS = (1, 2, 3, 4, 6)


def one_call(ctx, arenas, bid, n, step, timed):
    ids = np.ascontiguousarray([arenas[(step + j) % len(arenas)] for j in range(n)], dtype=np.uint64)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.probe_many(ids, bid, _lib.PROBE_ASYNC | (_lib.PROBE_TIMED if timed else 0))
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e6
    if not timed:
        return wall
    tm = ctx.timing_read(reset=True)
    return (tm.ms_terms_kernel + tm.ms_fused_kernel + tm.ms_eval_kernel) * 1e3, (tm.n_probe_arenas, tm.n_fused_arenas, tm.n_eval)


def run_configs(ctx, arenas, bid, configs, rounds, warm=2):
    """configs: [(name, n_arenas, key)] -> {name: ([kernel us], [wall us])}; one call of every configuration per round, in turn"""
    out = {c[0]: ([], []) for c in configs}
    step = 0
    for i in range(warm + rounds):
        for name, n, key in configs:
            if key is not None:
                ctx.set_lab(27, key)
            kern, counts = one_call(ctx, arenas, bid, n, step, True)
            assert counts[0] + counts[1] == n and counts[2] == 1, (name, counts)
            step += n
            wall = one_call(ctx, arenas, bid, n, step, False)
            step += n
            if i >= warm:
                out[name][0].append(kern)
                out[name][1].append(wall)
    return out


def med(v):
    return "%7.1f (%7.1f .. %7.1f)" % (float(np.median(v)), min(v), max(v))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "grid"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    print("library %s" % _lib.LIB_PATH, flush=True)
    bench.start_pool(16)
    ctx = Context((0,))
    ctx.set_lab(3, 0)
    ctx.set_timed_stride(1)
    try:
        ctx.set_lab(27, 0)
        has_key = True
    except Exception:
        has_key = False
    arenas, B = c2_arenas(ctx)
    bid, nq, nt = batch_of(ctx, synth.make_queries(4096, "c2", seed=1234))
    print("C2: %d queries, %d distinct terms, arenas of %d blocks, %d replicas; key 27 %s" % (nq, nt, B, len(arenas), "known" if has_key else "unknown: one chunk only"))
    if mode == "grid":
        arenas_list = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else ARENAS
        chunk_list = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else CHUNKS
        for n in arenas_list:
            configs = [("%d chunk%s%s%s" % (c, "" if c == 1 else "s", "" if c == 1 else ", eval " + ("spread" if place == 2 else "in front"), ", short last" if pct else ""),
                        n, (c | (pct << 16) | (place << 24)) if has_key else None)
                       for c in chunk_list for place in (1, 2) for pct in (0, 50) if (c > 1 or (pct == 0 and place == 1)) and (has_key or c == 1)]
            res = run_configs(ctx, arenas, bid, configs, rounds)
            print("%d arenas per call: us, median (min .. max) of %d calls each" % (n, rounds))
            base = float(np.median(res[configs[0][0]][1]))
            for name, _, _ in configs:
                k, w = res[name]
                print("  %-40s kernels %s   wall %s   per arena %.2f   vs one chunk %+.1f %%"
                      % (name, med(k), med(w), float(np.median(w)) / n, (float(np.median(w)) / base - 1) * 100), flush=True)
    elif mode == "default":
        for n in ARENAS:
            res = run_configs(ctx, arenas, bid, [("key 27 = 1", n, 1), ("key 27 = 0", n, 0)], rounds)
            for name in ("key 27 = 1", "key 27 = 0"):
                print("%3d arenas  %-11s kernels %s   wall %s" % (n, name, med(res[name][0]), med(res[name][1])), flush=True)
    else:
        sys.exit(__doc__)
    bench.stop_pool()


if __name__ == "__main__":
    main()
