"""Worker of test_eval_rows_gpu.py (run as a script in a process of its own: BSG_LAB_EVAL_ROWS and BSG_LAB_EVAL_TILE are read
once per process).  Runs every case of CASES on one context and writes {case: "ok" | what differs} as JSON to argv[1].

Expected survivors: the CPU oracle's probe_batch, computed by the first worker that needs them and kept in argv[2] (a directory
the test owns) for the workers after it, so every mode is held to the same arrays.

Arenas of 20-row blocks (the evaluator sees 64-block groups, not rows), every block from its own rows."""
import json
import os
import sys

import numpy as np

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.arena import plan_blocks
from bloomsearch_amd.gpu import Context
from oracle import oracle as O
from tests import helpers as H

ROWS = 20
BLOCKS = [1, 63, 64, 65, 511, 512, 513, 1000, 1023, 1024, 1025, 1100, 2049]      # G = 1, 1, 1, 2, 8, 8, 9, 16, 16, 16, 17, 18, 33
QUERIES = [1, 2, 255, 256, 257, 600]
TERMS = [3, 29, 64, 65, 77]
MIXED = [1000, 65, 1, 1025]
MIXED5 = [1000, 65, 1, 1025, 513]

_sets, _arenas = {}, {}


def arena(ctx, n_blocks, first=0):
    if (n_blocks, first) not in _arenas:
        for b in range(first, first + n_blocks):
            if b not in _sets:
                _sets[b] = synth.block_entry_sets(b * ROWS, ROWS)
        plan = plan_blocks([_sets[b] for b in range(first, first + n_blocks)], 0.001)
        _arenas[(n_blocks, first)] = (ctx.build(plan.blob, plan.off, plan.fstart, plan.desc, plan.n_words), plan.desc)
    return _arenas[(n_blocks, first)]


LEAVES = [Q.FieldToken("level", v) for v in synth.LEVELS] + [Q.FieldToken("service", v) for v in synth.SERVICES] + \
         [Q.FieldToken("nested.region", "region-%d" % i) for i in range(8)] + [Q.FieldToken("service", "absent-svc-%d" % i) for i in range(60)]


def c2_like(n):
    """n queries: three-term Ands over present and absent values, an Or and a nil query among them where there is room"""
    out = [Q.And(LEAVES[i % 4], LEAVES[len(synth.LEVELS) + i % 5], LEAVES[len(synth.LEVELS) + len(synth.SERVICES) + i % 9]) for i in range(n)]
    if n >= 3:
        out[1] = Q.Or(Q.FieldToken("level", "error"), Q.FieldToken("service", "absent-svc-2"))
        out[n - 1] = None
    return out


def nested(depth, i=0):
    """And(a, Or(b, And(c, ...))) of `depth` leaves: a postfix program whose stack grows to `depth`"""
    if depth == 1:
        return LEAVES[i % 12]
    return (Q.And if i % 2 == 0 else Q.Or)(LEAVES[i % 12], nested(depth - 1, i + 1))


def n_terms(n):
    """a batch of exactly n distinct terms: each alone, an And and an Or over the first, middle and last"""
    t = LEAVES[:n]
    return t + [Q.And(t[0], t[-1]), Q.Or(t[n // 2], t[-1]), Q.And(t[0], Q.Or(t[n // 2], t[-1]))]


PROGRAMS = {
    "nil": [None, None, None],
    "single": [LEAVES[0], LEAVES[5], LEAVES[30]],
    "and3": c2_like(40)[:1] + c2_like(40)[2:39],
    "or8": [Q.Or(*LEAVES[i: i + 8]) for i in range(0, 24, 3)] + [Q.Or(*LEAVES[20:28])],
    "mixed4": [nested(4, i) for i in range(12)] + [None, LEAVES[2]],
    "deep7": [nested(7, i) for i in range(5)] + c2_like(5),        # beyond what k_gather_fused gives a row span: the old body there
    "deep9": [nested(9, i) for i in range(5)] + c2_like(5),        # beyond the row span's and the tile's LDS anywhere: the per-group walk
}


def run_plain(ctx, aids, bid, nq, n_blocks):
    return ctx.probe_many(aids, bid, 0, nq, n_blocks)


def run_sentinel(ctx, aids, bid, nq, n_blocks):
    """the out-parameter form into a page-locked buffer longer than the survivors, filled with a sentinel: the call writes each
    arena's n_queries x G words and not one word more"""
    G = [(nb + 63) // 64 for nb in n_blocks]
    total, pad = nq * sum(G), 96
    out = ctx.pinned_array((total + pad) * 8).view(np.uint64)
    try:
        out[:] = np.uint64(0xA5A5A5A5DEADBEEF)
        ctx.probe_many_into(aids, bid, out[: total], 0)
        assert (out[total:] == np.uint64(0xA5A5A5A5DEADBEEF)).all(), "words beyond the last arena's n_queries x G were written"
        res, o = [], 0
        for g in G:
            res.append(out[o: o + nq * g].reshape(nq, g).copy())
            o += nq * g
        return res
    finally:
        ctx.pinned_free(out.view(np.uint8))


def check(ctx, want_dir, name, arenas, exprs, run=run_plain, key27=None, gather_cost=None, route=None):
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    terms = H.gpu_terms(ctx, cb)
    nq = len(exprs)
    path = os.path.join(want_dir, name.replace("/", "_") + ".npz")
    if os.path.exists(path):
        with np.load(path) as z:
            want = [z["a%d" % i] for i in range(len(arenas))]
    else:
        cache = {}
        want = []
        for w, d in arenas:
            if id(w) not in cache:
                cache[id(w)] = O.probe_batch(w, d.view(O.DESC_DTYPE), terms.view(O.TERM_DTYPE), ops, poff)
            want.append(cache[id(w)])
        np.savez(path + ".tmp.npz", **{"a%d" % i: a for i, a in enumerate(want)})
        os.replace(path + ".tmp.npz", path)
    n_blocks = [len(d) // 3 for _, d in arenas]
    loaded = {}
    for w, d in arenas:
        if id(w) not in loaded:
            loaded[id(w)] = ctx.arena_load(w, d)
    aids = [loaded[id(w)] for w, _ in arenas]
    bid = ctx.batch_create(terms, ops, poff)
    try:
        ctx.set_lab(3, 0)                                     # no one-dispatch path: the evaluation is a dispatch of its own, or rides in k_gather_fused
        if gather_cost is not None:
            ctx.set_gather_cost(gather_cost)
        if key27 is not None:
            ctx.set_lab(27, key27)
        got = run(ctx, aids, bid, nq, n_blocks)
        if route is not None:
            assert ctx.last_probe_route() == route, "route %d, expected %d" % (ctx.last_probe_route(), route)
        for i in range(len(arenas)):
            assert got[i].shape == want[i].shape, "arena %d: shape %s, oracle %s" % (i, got[i].shape, want[i].shape)
            if not np.array_equal(got[i], want[i]):
                bad = np.argwhere(got[i] != want[i])
                raise AssertionError("arena %d (%d blocks): %d words differ from the oracle, first at query %d word %d: %#x, oracle %#x"
                                     % (i, n_blocks[i], len(bad), bad[0][0], bad[0][1], int(got[i][tuple(bad[0])]), int(want[i][tuple(bad[0])])))
    finally:
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        for a in loaded.values():
            ctx.arena_free(a)


def cases(ctx):
    """-> [(name, thunk taking (ctx, want_dir))] — the names are the test's parameters"""
    out = []

    def add(name, arenas_of, exprs_of, **kw):
        out.append((name, lambda c, wd: check(c, wd, name, arenas_of(c), exprs_of(), **kw)))

    for nb in BLOCKS:
        add("blocks-%d" % nb, lambda c, nb=nb: [arena(c, nb)], lambda: c2_like(257))
    for nq in QUERIES:
        for nb in (512, 1025):
            add("queries-%d-blocks-%d" % (nq, nb), lambda c, nb=nb: [arena(c, nb)], lambda nq=nq: c2_like(nq))
    for p in PROGRAMS:
        add("program-%s" % p, lambda c: [arena(c, 1025)], lambda p=p: PROGRAMS[p])
    for t in TERMS:
        add("terms-%d" % t, lambda c: [arena(c, 1025), arena(c, 65, first=40)], lambda t=t: n_terms(t))
    mixed = lambda c: [arena(c, nb, first=7 * i) for i, nb in enumerate(MIXED)]
    mixed5 = lambda c: [arena(c, nb, first=7 * i) for i, nb in enumerate(MIXED5)]
    add("mixed-group", mixed, lambda: c2_like(257))
    add("mixed-group-gathered", mixed, lambda: c2_like(257), gather_cost=0, route=_lib.ROUTE_GATHER)
    add("mixed-group-streamed", mixed, lambda: c2_like(257), gather_cost=1 << 20, route=_lib.ROUTE_STREAM)
    add("mixed-group-sentinel", mixed, lambda: c2_like(257), run=run_sentinel)
    add("130-arenas-of-65-blocks", lambda c: [arena(c, 65, first=3 * (i % 4)) for i in range(130)], lambda: c2_like(40))
    for chunks in (2, 3, 5):
        add("chunked-%d" % chunks, mixed5, lambda: c2_like(257), key27=chunks, gather_cost=0, route=_lib.ROUTE_GATHER_CHUNKED)
    add("chunked-3-deep7", mixed5, lambda: PROGRAMS["deep7"], key27=3, gather_cost=0, route=_lib.ROUTE_GATHER_CHUNKED)
    add("chunked-3-600-queries", mixed5, lambda: c2_like(600), key27=3, gather_cost=0, route=_lib.ROUTE_GATHER_CHUNKED)
    return out


def case_names():
    return [n for n, _ in cases(None)]


def main():
    out_path, want_dir = sys.argv[1], sys.argv[2]
    results = {}
    ctx = Context((0,))
    try:
        for name, thunk in cases(ctx):
            try:
                thunk(ctx, want_dir)
                results[name] = "ok"
            except AssertionError as e:
                results[name] = "differs: %s" % e
            # (anything else — a HIP error among them — ends the worker: nothing more runs on the device after a fault)
            with open(out_path + ".tmp", "w") as f:
                json.dump(results, f)
            os.replace(out_path + ".tmp", out_path)
    finally:
        ctx.close()
    print("eval rows worker: %d cases, %d ok" % (len(results), sum(v == "ok" for v in results.values())))


if __name__ == "__main__":
    main()
