"""The chunked gather (bsg_set_lab key 27): a single group whose few-term launch gathers is probed in chunks of consecutive arenas —
k_probe_gather on chunk 0, one k_gather_fused per further chunk (gather chunk i + the program evaluation of chunk i - 1 in one
dispatch), k_eval_programs on the last chunk — against the oracle and against the same call with key 27 = 1 (the two plain dispatches).

Every case asserts three things: the survivors equal the oracle's probe_batch; they equal the same call under key 27 = 1; and
bsg_lab_last_probe_route names the route that ran (ROUTE_GATHER_CHUNKED, or the old route where the planner must refuse).  Arenas
of 200-row blocks as in test_probe_gather_gpu.py; the gather cost is 0 throughout, so whatever has bytes gathers."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.gpu import rows_to_dense
from oracle import oracle as O
from tests import helpers as H
from tests.test_probe_gather_gpu import C2_LIKE, arena

pytestmark = pytest.mark.gpu

CHUNKED, PLAIN = _lib.ROUTE_GATHER_CHUNKED, _lib.ROUTE_GATHER
FRONT, SPREAD = 1 << 24, 2 << 24                             # key 27, bits 24-25: k_gather_fused's evaluation workgroups in front / spread
NIL = frozenset({(3, 2), (8, 2), (4, 1)})                     # (block, kind) pairs without a filter
_want_cache = {}


def mixed_arenas(ctx, n):
    """n arenas with block counts mixed from {1, 8, 64, 65, 130} and one with nil filters among them, each from its own rows"""
    counts = [65, 1, 130, 8, 64, 9, 130, 1, 65]
    return [arena(ctx, counts[i], absent=NIL if counts[i] == 9 else frozenset(), first=100 * i) for i in range(n)]


def batch_of(n):
    """n queries: C2-like Ands in turn, an Or and a None among them where there is room"""
    out = [C2_LIKE[i % len(C2_LIKE)] for i in range(n)]
    if n >= 3:
        out[1] = Q.Or(Q.FieldToken("level", "error"), Q.FieldToken("service", "absent-svc-2"))
        out[n - 1] = None
    return out


def run_sync(ctx, aids, bid, nq, n_blocks, flags=0):
    return ctx.probe_many(aids, bid, flags, nq, n_blocks)


def check(ctx, arenas, exprs, key, route=CHUNKED, run=run_sync, setup=None, want_key=None):
    """arenas: [(words, desc)].  The call under key 27 = 1 first (it leaves ROUTE_GATHER behind, or what `setup` makes of it), then
    under `key`: -> the survivors of the second."""
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    terms = H.gpu_terms(ctx, cb)
    nq = len(exprs)
    want = []
    for w, d in arenas:
        k = (id(w), want_key if want_key is not None else id(exprs))
        if k not in _want_cache:
            _want_cache[k] = (w, exprs, O.probe_batch(w, d.view(O.DESC_DTYPE), terms.view(O.TERM_DTYPE), ops, poff))
        want.append(_want_cache[k][2])
    n_blocks = [len(d) // 3 for _, d in arenas]
    loaded = {}
    for w, d in arenas:
        if id(w) not in loaded:
            loaded[id(w)] = ctx.arena_load(w, d)
    aids = [loaded[id(w)] for w, _ in arenas]
    bid = ctx.batch_create(terms, ops, poff)
    try:
        ctx.set_lab(3, 0)                                     # no one-dispatch path
        ctx.set_gather_cost(0)
        ctx.set_lab(27, 1)
        if route is None:                                     # a route that does not report: the getter must keep this plain call's
            run_sync(ctx, aids, bid, nq, n_blocks)
        if setup:
            setup(True)
        base = run(ctx, aids, bid, nq, n_blocks)
        base_route = ctx.last_probe_route()
        ctx.set_lab(27, key)
        got = run(ctx, aids, bid, nq, n_blocks)
        assert ctx.last_probe_route() == (base_route if route is None else route), (key, ctx.last_probe_route(), base_route)
        assert base_route != CHUNKED
        for i in range(len(arenas)):
            assert np.array_equal(got[i], want[i]), "survivors of arena %d under key 27 = %#x differ from the oracle" % (i, key)
            assert np.array_equal(got[i], base[i]), "survivors of arena %d under key 27 = %#x and = 1 differ" % (i, key)
    finally:
        if setup:
            setup(False)
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        for a in loaded.values():
            ctx.arena_free(a)
    return got


@pytest.mark.parametrize("n_arenas", [2, 3, 5, 9])
@pytest.mark.parametrize("chunks", [2, 3, "n"])
@pytest.mark.parametrize("place", [0, FRONT, SPREAD])
def test_groups_of_mixed_arenas(ctx, n_arenas, chunks, place):
    got = check(ctx, mixed_arenas(ctx, n_arenas), C2_LIKE, (n_arenas if chunks == "n" else chunks) | place)
    assert got[0].any() and not got[0].all()


def test_a_shorter_last_chunk(ctx):
    check(ctx, mixed_arenas(ctx, 9), C2_LIKE, 3 | (50 << 16))


def test_130_arenas_of_3_blocks(ctx):
    """more records than the kernel arguments hold, and chunk cuts (44 / 43 / 43, 19 / 19 / ...) off any multiple of 8 or 64"""
    three = [arena(ctx, 3, first=3 * i) for i in range(4)]
    group = [three[i % 4] for i in range(130)]
    check(ctx, group, C2_LIKE[:40], 3 | FRONT, want_key="c2-40")
    check(ctx, group, C2_LIKE[:40], 7 | SPREAD, want_key="c2-40")


@pytest.mark.parametrize("n_queries", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("place", [FRONT, SPREAD])
def test_query_counts_with_a_partial_and_an_odd_chunk(ctx, n_queries, place):
    check(ctx, mixed_arenas(ctx, 3), batch_of(n_queries), 3 | place)


@pytest.mark.parametrize("kinds", [2, 3])
def test_referenced_kinds(ctx, kinds):
    leaves = [[Q.FieldToken("level", "error"), Q.FieldToken("service", "nope"), Q.FieldToken("nested.az", "az-1")],
              [Q.Token("error"), Q.Token("auth"), Q.Token("absent-token")],
              [Q.Field("nested.az"), Q.Field("user_id"), Q.Field("no.such.field")]][:kinds]
    flat = [x for ls in leaves for x in ls]
    exprs = flat + [Q.And(*[ls[0] for ls in leaves]), Q.Or(*[ls[1] for ls in leaves]), Q.And(*[ls[2] for ls in leaves]), None]
    check(ctx, [arena(ctx, 65), arena(ctx, 8, first=300), arena(ctx, 130, first=200)], exprs, 3)


def test_survivors_left_on_the_device_copied_to_host_memory_and_as_rows(ctx):
    from tests.test_configs_gpu import HipMem
    arenas = mixed_arenas(ctx, 5)
    G = [(len(d) // 3 + 63) // 64 for _, d in arenas]

    def split(flat, nq):
        out, o = [], 0
        for g in G:
            out.append(flat[o: o + nq * g].reshape(nq, g).copy())
            o += nq * g
        return out

    def run_dev_async(ctx, aids, bid, nq, n_blocks):
        mem = HipMem(nq * sum(G) * 8)
        try:
            ctx.probe_many_dev(aids, bid, mem.ptr.value, _lib.PROBE_ASYNC)
            ctx.sync()
            return split(mem.read(), nq)
        finally:
            mem.free()

    def run_pinned_async(ctx, aids, bid, nq, n_blocks):
        out = ctx.pinned_array(nq * sum(G) * 8).view(np.uint64)
        try:
            out[:] = 0
            ctx.probe_many_into(aids, bid, out, _lib.PROBE_ASYNC)
            ctx.sync()
            return split(out, nq)
        finally:
            ctx.pinned_free(out.view(np.uint8))

    def run_rows(packed):
        def run(ctx, aids, bid, nq, n_blocks):
            rows = ctx.pinned_array(nq * sum(G) * 8).view(np.uint64)
            hdr = ctx.pinned_array(nq * len(G) * 4).view(np.uint32)
            try:
                ctx.probe_many_rows(aids, bid, rows, hdr, _lib.PROBE_ROWS_PACKED if packed else 0)
                h = hdr.view(np.uint8) if packed else hdr
                out, o = [], 0
                for i, g in enumerate(G):
                    out.append(rows_to_dense(h[i * nq: (i + 1) * nq], rows[o: o + nq * g], n_blocks[i], packed=packed))
                    o += nq * g
                return out
            finally:
                ctx.pinned_free(rows.view(np.uint8))
                ctx.pinned_free(hdr.view(np.uint8))
        return run

    for run in (run_dev_async, run_pinned_async, run_sync, run_rows(False), run_rows(True)):
        check(ctx, arenas, C2_LIKE, 3 | SPREAD, run=run)


def test_two_calls_with_different_chunk_counts_reuse_slot_and_table(ctx):
    arenas = mixed_arenas(ctx, 9)

    def run(ctx, aids, bid, nq, n_blocks):
        # a call in 4 chunks over the 9 arenas, one in 2 over the first 5, the 9 again in 2: same slot, another table
        # (check's first pass, under key 27 = 1: the same three calls, all plain)
        chunked = not ctx_key["plain"]
        if chunked:
            ctx.set_lab(27, 4)
        first = ctx.probe_many(aids, bid, 0, nq, n_blocks)
        if chunked:
            assert ctx.last_probe_route() == CHUNKED
            ctx.set_lab(27, 2)
        second = ctx.probe_many(aids[:5], bid, 0, nq, n_blocks[:5])
        again = ctx.probe_many(aids, bid, 0, nq, n_blocks)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)
        ctx_key["plain"] = False
        return first

    ctx_key = {"plain": True}
    check(ctx, arenas, C2_LIKE, 2, run=run)


def test_a_timed_call_counts_every_arena_once(ctx):
    def run(ctx, aids, bid, nq, n_blocks):
        ctx.timing_read(reset=True)
        got = ctx.probe_many(aids, bid, _lib.PROBE_TIMED, nq, n_blocks)
        t = ctx.timing_read()
        counts.append((t.n_probes, t.n_probe_arenas, t.n_fused, t.n_fused_arenas, t.n_eval, t.stream_bytes > 0, t.fused_stream_bytes > 0,
                       t.ms_terms_kernel > 0, t.ms_fused_kernel > 0, t.ms_eval_kernel > 0))
        return got

    counts = []
    check(ctx, mixed_arenas(ctx, 9), C2_LIKE, 4, run=run)
    assert counts[0] == (1, 9, 0, 0, 1, True, False, True, False, True)           # key 27 = 1: the two plain dispatches
    assert counts[1] == (1, 3, 3, 6, 1, True, True, True, True, True)             # 4 chunks of 3 / 2 / 2 / 2 arenas: 3 + 6 = the group


def test_a_many_term_batch_keeps_the_old_route(ctx):
    terms = [Q.FieldToken("service", "absent-svc-%d" % i) for i in range(140)] + [Q.FieldToken("level", "error")]
    exprs = terms + [Q.And(terms[0], terms[-1]), Q.Or(terms[7], terms[-1])]
    check(ctx, mixed_arenas(ctx, 3), exprs, 3, route=_lib.ROUTE_STREAM)


def test_a_batch_forced_to_stream_keeps_the_old_route(ctx):
    def setup(on):
        ctx.set_gather_cost(1 << 20 if on else _lib.GATHER_COST_DEFAULT)
    check(ctx, mixed_arenas(ctx, 3), C2_LIKE, 3, route=_lib.ROUTE_STREAM, setup=setup)


def test_a_multi_group_run_keeps_the_old_route(ctx):
    def setup(on):
        ctx.set_probe_group(2 if on else 0)
        ctx.set_fuse_limit(0 if on else 4)
    check(ctx, mixed_arenas(ctx, 5), C2_LIKE, 3, route=PLAIN, setup=setup)


@pytest.mark.parametrize("lab_key,value", [(19, 50), (11, 8)])
def test_runs_with_tail_split_or_fold_set_keep_the_old_route(ctx, lab_key, value):
    def setup(on):
        ctx.set_lab(lab_key, value if on else 0)
    # (key 11: the folded dispatch does not report a route of its own: the getter keeps what the call before it left)
    check(ctx, mixed_arenas(ctx, 9), C2_LIKE, 3, route=PLAIN if lab_key == 19 else None, setup=setup)
