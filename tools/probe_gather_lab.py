"""Lab: a few-term probe launch GATHERED (k_probe_gather: one wave per block reads the words it tests) against STREAMED (k_probe_terms:
every bitset through LDS) and against the per-block gathered path inside k_probe_terms, at the headline's launch shape: the bench's C2
arena (1 000 blocks x 10 000 rows, fpr 0.001) and batch, 20 arenas per dispatch over 16 rotating replicas, BSG_PROBE_TIMED.

    python tools/probe_gather_lab.py c2 [launches [routes]] kernel time per launch from the dispatch timestamps, the three routes interleaved
    python tools/probe_gather_lab.py sweep [launches]     distinct terms per kind {3 .. 128}: gather vs stream, product and big_filters geometry
    python tools/probe_gather_lab.py pmc ROUTE [launches [arenas [cap]]]
                                                          launches of ONE route and nothing else (under rocprofv3 --pmc FETCH_SIZE / TCC_EA0_RDREQ_sum)
    python tools/probe_gather_lab.py lines [--order A,B,..]
                                                          no GPU: the EXACT number of distinct 128-byte lines the executed bit tests of the bench's batch touch
                                                          per block of the bench's arena (in all, and summed phase by phase), and the tests executed, under
                                                          every phase schedule of the gather kernel and every order of a lane's k locations (ORDERS; default all)
    python tools/probe_gather_lab.py caps [rounds [arenas,.. [caps,..]]]
                                                          the gather route under bsg_set_lab key 28 = workgroups per CU (5 = no cap), the caps taking turns call by
                                                          call: kernel time (the dispatches' timestamps, summed) and call wall time, survivors left on the device

ROUTE: stream (bsg_set_gather_cost(1 << 20)), block (cost 0, bsg_set_lab key 26 = 0: k_probe_terms' per-block gathered path), gather (cost 0).
BSG_LAB_LIB=path loads another build of the library (the -DBSG_GATHER_* variants of csrc/kernels.hip.h).
The numbers on record and the stop rules they are read by: profiles/probe_gather_lab.txt, profiles/probe_gather_lines_lab.txt,
profiles/probe_gather_order_lab.txt.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bloomsearch_amd import _lib, query as Q, synth
if os.environ.get("BSG_LAB_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["BSG_LAB_LIB"])
from bloomsearch_amd.arena import plan_blocks
from bloomsearch_amd.gpu import Context, estimate_parameters
from benchlib import common as bench

ROUTES = {"stream": (1 << 20, 1, _lib.ROUTE_STREAM), "block": (0, 0, _lib.ROUTE_STREAM), "gather": (0, 1, _lib.ROUTE_GATHER)}
PER_CALL, R = 20, 16
PRESENT = [("level", v) for v in synth.LEVELS] + [("service", v) for v in synth.SERVICES] + [("nested.region", "region-%d" % i) for i in range(synth.N_REGIONS)] + \
          [("nested.az", "az-%d" % i) for i in range(synth.N_AZS)] + [(f, w) for f in ("tags", "message") for w in synth.WORDS]


def set_route(ctx, name):
    cost, kernel, _ = ROUTES[name]
    ctx.set_gather_cost(cost)
    ctx.set_lab(26, kernel)


def batch_of(ctx, exprs):
    cb = Q.compile_queries(exprs)
    ops, poff, kinds = cb.arrays()
    terms = np.zeros(len(cb.term_strings), dtype=_lib.TERM_DTYPE)
    terms["h"] = ctx.hash_strings(cb.term_strings)
    terms["kind"] = kinds
    return ctx.batch_create(terms, ops, poff), len(exprs), len(terms)


def c2_arenas(ctx):
    """the bench's arena, R replicas.  BSG_LAB_CACHE=dir keeps the built words between runs of this script (generation is most of a run)."""
    B, rows = 1000, 10000
    cache = os.environ.get("BSG_LAB_CACHE")
    files = [os.path.join(cache, "c2_%s.npy" % n) for n in ("words", "desc")] if cache else []
    if cache and all(os.path.exists(f) for f in files):
        words, desc = np.load(files[0]), np.load(files[1])
    else:
        plan = plan_blocks(bench.generate_blocks(np.arange(B, dtype=np.int64), rows, 0xB100F5EA4C4, 16), 0.001)
        words, desc = ctx.build(plan.blob, plan.off, plan.fstart, plan.desc, plan.n_words), plan.desc
        if cache:
            os.makedirs(cache, exist_ok=True)
            np.save(files[0], words)
            np.save(files[1], desc)
    return [ctx.arena_load(words, desc) for _ in range(R)], B


def big_arenas(ctx):
    """benchlib.legs.big_filter_leg's geometry: 64 blocks x one 1.04 MB token filter, 4 replicas."""
    n_blocks, per_block = 64, 580_000
    m, k = estimate_parameters(per_block, 0.001)
    stride = ((m + 63) // 64 + 15) // 16 * 16
    toks = np.random.default_rng(20260927).integers(1, 1 << 62, size=n_blocks * per_block, dtype=np.uint64)
    off = (np.arange(n_blocks * per_block + 1, dtype=np.uint64) * 8).astype(np.uint32)
    desc = np.zeros(n_blocks * 3, dtype=_lib.DESC_DTYPE)
    fstart = [0]
    for b in range(n_blocks):
        fstart.append(b * per_block)
        desc[b * 3 + 1] = (b * stride, m, k, 0)
        fstart += [(b + 1) * per_block, (b + 1) * per_block]
    words = ctx.build(toks.view(np.uint8), off, np.asarray(fstart, dtype=np.uint32), desc, n_blocks * stride)
    return [ctx.arena_load(words, desc) for _ in range(4)], n_blocks


def time_routes(ctx, arenas, bid, per_call, routes, launches, warm=3):
    """-> {route: [kernel us per launch]}: the routes take turns launch by launch, each launch on the next replicas in rotation."""
    flags = _lib.PROBE_TIMED | _lib.PROBE_ASYNC | _lib.PROBE_NOFUSE
    out = {r: [] for r in routes}
    step = 0
    for i in range(warm + launches):
        for r in routes:
            set_route(ctx, r)
            ids = np.ascontiguousarray([arenas[(step + j) % len(arenas)] for j in range(per_call)], dtype=np.uint64)
            step += per_call
            ctx.probe_many(ids, bid, flags)
            ctx.sync()
            tm = ctx.timing_read(reset=True)
            assert ctx.last_probe_route() == ROUTES[r][2], (r, ctx.last_probe_route())
            if i >= warm:
                out[r].append(tm.ms_terms_kernel / max(tm.n_probes, 1) * 1e3)
    return out


SCHEDULES = ((4, 4, 2), (2, 8), (2, 2, 6), (4, 6), (1, 3, 6), (10,))
ORDERS = ("index", "line", "zones", "count_zone", "count_line")


def phase_of_position(sch, kmax):
    """-> [kmax] the phase that takes the lane's j-th location under the schedule (the last length repeats beyond the list)"""
    ph, at, p = np.zeros(kmax, dtype=np.int64), 0, 0
    while at < kmax:
        ph[at: at + sch[min(p, len(sch) - 1)]] = p
        at += sch[min(p, len(sch) - 1)]
        p += 1
    return ph


def gather_locations(words, desc, h, kinds):
    """words / desc of one arena, h [T][4] base hashes, kinds [T] -> x [T][kmax] the raw locations, and per [B][T][kmax]: live (i < k of a
    filter that is not nil), loc (x mod m), bit (the filter's bit there; True where not live), line (the 128-byte line of the arena)"""
    B = len(desc) // 3
    d = desc.reshape(B, 3)
    m = d["m"][:, kinds].astype(np.uint64)                                # [B][T]
    k = d["k"][:, kinds].astype(np.int64)
    base = d["word_off"][:, kinds].astype(np.uint64)
    kmax = int(k.max())
    i = np.arange(kmax)
    with np.errstate(over="ignore"):
        x = h[:, i % 2] + i.astype(np.uint64)[None, :] * h[:, 2 + ((i + i % 2) % 4) // 2]       # bloom/v3 location(h, i), wrapping u64: [T][k]
    live = (m > 0)[:, :, None] & (i[None, None, :] < k[:, :, None])
    loc = x[None, :, :] % np.maximum(m, 1)[:, :, None]                    # [B][T][k]
    bit = ((words[(base[:, :, None] + (loc >> np.uint64(6))).astype(np.int64)] >> (loc & np.uint64(63))) & np.uint64(1)).astype(bool) | ~live
    line = ((base[:, :, None] * np.uint64(8) + (loc >> np.uint64(3))) >> np.uint64(7)).astype(np.int64)
    return x, live, loc, bit, line, m, k


def order_of(order, sch, live, loc, line, m, k):
    """-> perm [B][T][kmax]: the hash index of the location a lane tests at position j.  Every order is a total order (ties by hash
    index) and puts the positions beyond k last.
      index       the hash index: the kernel as built with BSG_GATHER_ORDER=0
      line        ascending 128-byte span of the filter (loc >> 10), ties by hash index: BSG_GATHER_ORDER=1
      zones       the filter's address range cut in the proportions of the phase lengths (1,3,6: 10 % / 30 % / 60 %); a location wants the
                  phase of its zone, a full phase spills into the next, an empty slot takes from the next zone: a stable sort by zone
      count_zone  with the wave's count of locations per line (all lanes, all k): the locations on lines wanted more than once go, in line
                  order, to the phase of their zone (the next free phase after it, else the latest free one before it); the others fill the latest free slots
      count_line  the locations on lines wanted more than once first, in line order; the others after them in index order"""
    B, T, kmax = loc.shape
    idx = np.broadcast_to(np.arange(kmax), loc.shape)
    dead = ~live
    rel = (loc >> np.uint64(10)).astype(np.int64)                         # the 128-byte span of the filter (filters start on 16-byte boundaries: not quite the arena's line)
    ph = phase_of_position(sch, kmax)
    if order == "index":
        return np.lexsort((idx, dead))
    if order == "line":
        return np.lexsort((idx, rel, dead))
    kk = np.maximum(k, 1)[:, :, None]
    zone = ph[np.minimum(loc.astype(np.int64) * kk // np.maximum(m, 1).astype(np.int64)[:, :, None], kk - 1)]
    if order == "zones":
        return np.lexsort((idx, zone, dead))
    shared = np.zeros(loc.shape, dtype=bool)                              # the wave: the lanes (terms) of one block and kind share the filter
    for b in range(B):
        u, inv, cnt = np.unique(line[b][live[b]], return_inverse=True, return_counts=True)
        shared[b][live[b]] = cnt[inv] > 1
    if order == "count_line":
        return np.lexsort((idx, np.where(shared, rel, 0), ~shared, dead))
    assert order == "count_zone", order
    perm = np.lexsort((idx, dead))
    by_line = np.lexsort((idx, rel, dead))
    n_ph = int(ph.max()) + 1
    for b in range(B):
        for t in range(T):
            n = int(live[b, t].sum())
            if n == 0:
                continue
            free = [[j for j in range(n) if ph[j] == p] for p in range(n_ph)]
            out = [0] * n
            for i in by_line[b, t, :n]:
                if shared[b, t, i]:
                    z = int(zone[b, t, i])
                    p = next((q for q in range(z, n_ph) if free[q]), None)
                    if p is None:
                        p = next(q for q in range(z - 1, -1, -1) if free[q])
                    out[free[p].pop(0)] = i
            for i in range(n):
                if not shared[b, t, i]:
                    p = next(q for q in range(n_ph - 1, -1, -1) if free[q])
                    out[free[p].pop()] = i
            perm[b, t, :n] = out
    return perm


def phase_walk(sch, perm, live, bit, line):
    """The kernel's phase walk over the locations in the order perm: a lane runs a phase iff every bit of its earlier phases was set.
    -> ran [B][T][kmax] (by position), the lines by position, the phase of each position"""
    kmax = perm.shape[2]
    ph = phase_of_position(sch, kmax)
    start = np.asarray([int(np.argmax(ph == ph[j])) for j in range(kmax)])
    bit_p, live_p, line_p = (np.take_along_axis(a, perm, axis=2) for a in (bit, live, line))
    passed = np.concatenate([np.ones(bit_p.shape[:2] + (1,), dtype=bool), np.logical_and.accumulate(bit_p, axis=2)], axis=2)   # [.., j]: bits 0 .. j - 1 all set
    return passed[:, :, start] & live_p, line_p, ph


def touched_lines(words, desc, h, kinds, schedules, orders=("index",)):
    """The gather kernel's loads, restated -> {(order, schedule): (tests executed, distinct 128-byte lines, sum over the phases of the
    phase's distinct lines), each per block}, the raw locations, the verdicts.  The distinct lines are the requests if every line a
    later phase wants again is still in the L2, the per-phase sum if none is; duplicates inside a phase merge either way."""
    x, live, loc, bit, line, m, k = gather_locations(words, desc, h, kinds)
    B = live.shape[0]
    out = {}
    for order in orders:
        for sch in schedules:
            ran, line_p, ph = phase_walk(sch, order_of(order, sch, live, loc, line, m, k), live, bit, line)
            n_ph = int(ph.max()) + 1
            out[(order, sch)] = (ran.sum() / B, len(np.unique(line_p[ran])) / B, len(np.unique((line_p * n_ph + ph[None, None, :])[ran])) / B)
    return out, x, bit.all(axis=2)


def lines_arena(B, rows):
    """the bench's arena built by the CPU oracle -> words, desc.  BSG_LAB_CACHE=dir keeps it between runs, as c2_arenas does."""
    from oracle import oracle as O
    cache = os.environ.get("BSG_LAB_CACHE")
    files = [os.path.join(cache, "lines_%d_%d_%s.npy" % (B, rows, n)) for n in ("words", "desc")] if cache else []
    if cache and all(os.path.exists(f) for f in files):
        return np.load(files[0]), np.load(files[1])
    plan = plan_blocks(bench.generate_blocks(np.arange(B, dtype=np.int64), rows, 0xB100F5EA4C4, 16), 0.001)
    words = O.build_many(plan.blob, plan.off, plan.fstart, plan.desc.view(O.DESC_DTYPE), plan.n_words)
    if cache:
        os.makedirs(cache, exist_ok=True)
        np.save(files[0], words)
        np.save(files[1], plan.desc)
    return words, plan.desc


def fmt(v):
    return "median %7.1f us  (min %7.1f, max %7.1f, spread %5.1f, n = %d)" % (float(np.median(v)), min(v), max(v), max(v) - min(v), len(v))


def same_results(ctx, arenas, bid, nq, n_blocks, routes):
    ref = None
    for r in routes:
        set_route(ctx, r)
        got = ctx.probe_many(arenas[:2], bid, _lib.PROBE_NOFUSE, nq, [n_blocks] * 2)
        if ref is None:
            ref = got
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "route %s differs" % r


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
    bench.start_pool(16)         # the synthetic generator's workers: forked before the HIP runtime exists here
    if mode == "lines":          # the CPU oracle alone: its filters, its hashes, its location arithmetic
        from oracle import oracle as O
        B, rows = 1000, 10000
        words, desc = lines_arena(B, rows)
        bench.stop_pool()
        cb = Q.compile_queries(synth.make_queries(4096, "c2", seed=1234))
        kinds = np.asarray(cb.arrays()[2], dtype=np.int64)
        h = np.asarray([O.base_hashes(s if isinstance(s, bytes) else s.encode()) for s in cb.term_strings], dtype=np.uint64)
        orders = ORDERS if "--order" not in sys.argv else tuple(sys.argv[sys.argv.index("--order") + 1].split(","))
        assert all(o in ORDERS for o in orders), "--order takes a comma-separated list of %s" % (ORDERS,)
        res, x, verdict = touched_lines(words, desc, h, kinds, SCHEDULES, orders)
        for t in range(len(h)):
            for i in range(x.shape[1]):
                assert int(x[t, i]) == O.location(tuple(int(v) for v in h[t]), i)
        d2 = desc.reshape(B, 3)
        n_present = int((verdict.mean(axis=0) > 0.5).sum())
        print("bench arena (%d blocks x %d rows, fpr 0.001) and batch (%d distinct terms, %d of them pass in most blocks, kinds %s); field::token filters of %.1f lines, k = %d"
              % (B, rows, len(h), n_present, sorted(set(kinds.tolist())), float(np.mean((d2["m"][:, 2] + 1023) // 1024)), int(d2["k"][:, 2].max())))
        print("per block: tests executed / distinct lines touched (requests if every cross-phase reuse hits) / sum of the phases' distinct lines (if none hits) / midpoint")
        for (order, sch), (tests, lines, per_phase) in res.items():
            print("  order %-10s schedule %-8s tests %6.1f   distinct lines %6.1f   per-phase sum %6.1f   midpoint %6.1f"
                  % (order, ",".join(map(str, sch)), tests, lines, per_phase, (lines + per_phase) / 2), flush=True)
        return
    print("library %s" % _lib.LIB_PATH, flush=True)
    ctx = Context((0,))
    ctx.set_lab(3, 0)            # no one-dispatch path: every launch goes through k_probe_terms / k_probe_gather
    ctx.set_timed_stride(1)
    if mode == "c2":
        launches = int(sys.argv[2]) if len(sys.argv) > 2 else 24
        arenas, B = c2_arenas(ctx)
        bid, nq, nt = batch_of(ctx, synth.make_queries(4096, "c2", seed=1234))
        routes = sys.argv[3].split(",") if len(sys.argv) > 3 else ["stream", "block", "gather"]
        same_results(ctx, arenas, bid, nq, B, routes)
        print("C2: %d queries, %d distinct terms, %d arenas of %d blocks per dispatch, %d replicas; survivors identical on all routes" % (nq, nt, PER_CALL, B, R))
        for r, v in time_routes(ctx, arenas, bid, PER_CALL, routes, launches).items():
            print("  %-7s %s" % (r, fmt(v)), flush=True)
    elif mode == "pmc":
        route, launches = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8
        per_call = int(sys.argv[4]) if len(sys.argv) > 4 else PER_CALL
        arenas, B = c2_arenas(ctx)
        bid, nq, nt = batch_of(ctx, synth.make_queries(4096, "c2", seed=1234))
        set_route(ctx, route)
        if len(sys.argv) > 5:
            ctx.set_lab(28, int(sys.argv[5]))
        for i in range(launches):
            ctx.probe_many(np.ascontiguousarray([arenas[(i * per_call + j) % R] for j in range(per_call)], dtype=np.uint64), bid, _lib.PROBE_ASYNC | _lib.PROBE_NOFUSE)
            ctx.sync()
        print("pmc: %d launches of %d arenas (%d blocks each) on route %s, key 28 = %s" % (launches, per_call, B, route, sys.argv[5] if len(sys.argv) > 5 else "default"))
    elif mode == "caps":
        import time
        rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 16
        counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [20, 200]
        caps = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [5, 3, 2, 1]
        arenas, B = c2_arenas(ctx)
        bid, nq, nt = batch_of(ctx, synth.make_queries(4096, "c2", seed=1234))
        set_route(ctx, "gather")
        try:
            ctx.set_lab(28, 0)
            has_key = True
        except Exception:                 # a build from before key 28: its one configuration
            has_key, caps = False, [5]
        step = 0
        for n in counts:
            kern, wall = {c: [] for c in caps}, {c: [] for c in caps}
            for i in range(2 + rounds):
                for c in caps:
                    if has_key:
                        ctx.set_lab(28, c)
                    for timed in (True, False):
                        ids = np.ascontiguousarray([arenas[(step + j) % R] for j in range(n)], dtype=np.uint64)
                        step += n
                        ctx.sync()
                        t0 = time.perf_counter()
                        ctx.probe_many(ids, bid, _lib.PROBE_ASYNC | (_lib.PROBE_TIMED if timed else 0))
                        ctx.sync()
                        w = (time.perf_counter() - t0) * 1e6
                        if timed:
                            tm = ctx.timing_read(reset=True)
                            assert ctx.last_probe_route() in (_lib.ROUTE_GATHER, _lib.ROUTE_GATHER_CHUNKED)
                            if i >= 2:
                                kern[c].append((tm.ms_terms_kernel + tm.ms_fused_kernel) * 1e3)
                        elif i >= 2:
                            wall[c].append(w)
            print("%d arenas per call, route %d (us; probe and fused dispatches' own time, and the call's wall time with no timestamps):" % (n, ctx.last_probe_route()))
            for c in caps:
                print("  key 28 = %d   gather dispatches %s   wall %s" % (c, fmt(kern[c]), fmt(wall[c])), flush=True)
    elif mode == "sweep":
        launches = int(sys.argv[2]) if len(sys.argv) > 2 else 12
        for name, (arenas, B), per_call, field in (("product geometry: 1 000-block arenas, 20 per launch", c2_arenas(ctx), PER_CALL, "nested.region"),
                                                   ("big_filters geometry: 64 blocks x 1.04 MB, 8 arenas per launch", big_arenas(ctx), 8, None)):
            print(name, flush=True)
            mixes = [(T, None) for T in (3, 8, 16, 29, 32, 36, 48, 64, 77, 128)]
            if field and os.environ.get("BSG_LAB_SWEEP") == "near":       # only the rows around the crossover, C2's mix and every term present
                mixes = [(T, None) for T in (29, 32, 36)] + [(T, T) for T in (29, 32, 36)]
            elif field:
                mixes += [(T, T) for T in (29, 32, 36)]                   # ... and every term present in every block: the dearest batch for the two-phase kernel
            elif os.environ.get("BSG_LAB_SWEEP") == "near":
                mixes = []
            for T, forced in mixes:
                if field:
                    # C2's mix where the generator allows it: three terms in four occur in every block (the synthetic rows hold 46 such
                    # field::token values), the rest in none; an absent term dies after the first batch of locations, a present one pays all k
                    n_present = forced if forced is not None else min(len(PRESENT), (3 * T + 3) // 4)
                    bid, nq, nt = batch_of(ctx, [Q.FieldToken(f, v) for f, v in PRESENT[:n_present]] + [Q.FieldToken(field, "region-%d" % (100 + i)) for i in range(T - n_present)])
                else:
                    bid, nq, nt = batch_of(ctx, [Q.Token("tok-%d" % i) for i in range(T)])
                assert nt == T
                same_results(ctx, arenas, bid, nq, B, ["stream", "gather"])
                t = time_routes(ctx, arenas, bid, per_call, ["stream", "gather"], launches)
                s, g = float(np.median(t["stream"])), float(np.median(t["gather"]))
                print("  terms %3d (%2d in every block)   stream %8.1f us (%.1f .. %.1f)   gather %8.1f us (%.1f .. %.1f)   gather / stream %.2f"
                      % (T, n_present if field else 0, s, min(t["stream"]), max(t["stream"]), g, min(t["gather"]), max(t["gather"]), g / s), flush=True)
                ctx.batch_free(bid)
            for a in arenas:
                ctx.arena_free(a)
    else:
        sys.exit(__doc__)
    bench.stop_pool()


if __name__ == "__main__":
    main()
