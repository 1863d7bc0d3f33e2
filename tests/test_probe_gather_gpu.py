"""k_probe_gather (one wave per block reads the words it tests straight from the arena) against the oracle and against the streamed
k_probe_terms, on every shape at which the gather kernel takes another path: partial workgroups (8 blocks each) and partial 64-block
verdict groups, one / two term words and a padded tail, grid y of 1-3 kinds, k of 1 / 2 / 10 / 20 (less and more than one load batch), filters of a
few words, a nil filter among real ones, grouped launches (records in the kernel arguments and in device memory), a filter beyond
2^31 bits (the 64-bit modulo), and the asynchronous and survivor-row calls the verdict words feed.

Every case asserts: survivors under bsg_set_gather_cost(0) == the oracle's probe_batch == survivors under bsg_set_gather_cost(1 << 20),
and bsg_lab_last_probe_route names the gather kernel for the first and the streaming kernels for the second."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd._lib import DESC_DTYPE
from bloomsearch_amd.arena import plan_blocks
from bloomsearch_amd.gpu import pack_entries, rows_to_dense
from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROWS = 200
_arena_cache = {}


def arena(ctx, n_blocks, rows=ROWS, fpr=0.001, absent=frozenset(), first=0):
    """-> (words, desc): built once per geometry and shared by the cases (never changed)."""
    key = (n_blocks, rows, fpr, tuple(sorted(absent)), first)
    if key not in _arena_cache:
        plan = plan_blocks([synth.block_entry_sets((first + b) * rows, rows) for b in range(n_blocks)], fpr, absent=set(absent))
        _arena_cache[key] = (ctx.build(plan.blob, plan.off, plan.fstart, plan.desc, plan.n_words), plan.desc)
    return _arena_cache[key]


def field_token_terms(n):
    """n distinct field::token terms, present and absent values mixed"""
    present = [("level", v) for v in synth.LEVELS] + [("service", v) for v in synth.SERVICES] + [("nested.region", "region-%d" % i) for i in range(8)] + \
              [("nested.az", "az-%d" % i) for i in range(3)]
    out = []
    for i in range(n):
        out.append(present[i // 2] if i % 2 == 0 and i // 2 < len(present) else ("service", "absent-svc-%d" % i))
    assert len(set(out)) == n
    return [Q.FieldToken(f, t) for f, t in out]


def check_routes(ctx, arenas, exprs, run=None):
    """arenas: [(words, desc)].  run(aids, bid, nq, n_blocks) -> [survivors per arena]; default: one synchronous bsg_probe_many."""
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    terms = H.gpu_terms(ctx, cb)
    nq = len(exprs)
    want = [O.probe_batch(w, d.view(O.DESC_DTYPE), terms.view(O.TERM_DTYPE), ops, poff) for w, d in arenas]
    n_blocks = [len(d) // 3 for _, d in arenas]
    aids = [ctx.arena_load(w, d) for w, d in arenas]
    bid = ctx.batch_create(terms, ops, poff)
    if run is None:
        run = lambda aids, bid, nq, n_blocks: ctx.probe_many(aids, bid, 0, nq, n_blocks)
    try:
        ctx.set_lab(3, 0)                                    # no one-dispatch path: the probe is a dispatch of its own
        got = {}
        for cost, route in ((0, _lib.ROUTE_GATHER), (1 << 20, _lib.ROUTE_STREAM)):
            ctx.set_gather_cost(cost)
            got[cost] = run(aids, bid, nq, n_blocks)
            assert ctx.last_probe_route() == route, (cost, ctx.last_probe_route())
        for i in range(len(arenas)):
            assert np.array_equal(got[0][i], want[i]), "gathered survivors of arena %d differ from the oracle" % i
            assert np.array_equal(got[0][i], got[1 << 20][i]), "gathered and streamed survivors of arena %d differ" % i
    finally:
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        for a in aids:
            ctx.arena_free(a)
    return want


C2_LIKE = [Q.And(Q.FieldToken("level", lv), Q.FieldToken("service", sv), Q.FieldToken("nested.region", "region-%d" % r))
           for lv in synth.LEVELS + ["absent-level-1"] for sv in synth.SERVICES[:3] + ["absent-svc-2"] for r in (0, 3, 7, 9)]


@pytest.mark.parametrize("n_blocks", [1, 7, 8, 9, 63, 64, 65, 130])
def test_block_counts(ctx, n_blocks):
    want = check_routes(ctx, [arena(ctx, n_blocks)], C2_LIKE)
    assert want[0].any() and not want[0].all()               # the batch prunes some (query, block) pairs and keeps others


@pytest.mark.parametrize("n_terms", [1, 29, 64, 65, 128])
def test_distinct_terms_per_kind(ctx, n_terms):
    terms = field_token_terms(n_terms)
    exprs = terms + [Q.And(terms[0], terms[-1]), Q.Or(terms[n_terms // 2], terms[-1])]
    check_routes(ctx, [arena(ctx, 65)], exprs)


@pytest.mark.parametrize("kinds", [1, 2, 3])
def test_referenced_kinds(ctx, kinds):
    leaves = [[Q.FieldToken("level", "error"), Q.FieldToken("service", "nope"), Q.FieldToken("nested.az", "az-1")],
              [Q.Token("error"), Q.Token("auth"), Q.Token("absent-token")],
              [Q.Field("nested.az"), Q.Field("user_id"), Q.Field("no.such.field")]][:kinds]
    flat = [x for ls in leaves for x in ls]
    exprs = flat + [Q.And(*[ls[0] for ls in leaves]), Q.Or(*[ls[1] for ls in leaves]), Q.And(*[ls[2] for ls in leaves]), None]
    check_routes(ctx, [arena(ctx, 65)], exprs)


@pytest.mark.parametrize("fpr,k", [(0.7, 1), (0.5, 2), (0.001, 10), (1e-6, 20)])
def test_k_of_1_2_10_and_20(ctx, fpr, k):
    """fpr 0.5 / 0.001 / 1e-6 give k = 2 / 10 / 20 (bloom/v3 EstimateParameters rounds ln 2 x m / n up); 0.7 gives the k = 1 that 0.5 was
    meant to: less than one load batch, one batch exactly is inside 10, and 20 is five of them"""
    words, desc = arena(ctx, 9, fpr=fpr)
    assert int(desc["k"][2]) == k                             # (block 0's field::token filter)
    check_routes(ctx, [(words, desc)], C2_LIKE)


def test_filters_of_a_few_words(ctx):
    words, desc = arena(ctx, 65, rows=3)
    assert int(desc["m"][2::3].max()) < 64 * 64               # every field::token filter within a few sectors
    check_routes(ctx, [(words, desc)], C2_LIKE)


def test_a_nil_filter_among_real_ones(ctx):
    words, desc = arena(ctx, 9, absent=frozenset({(3, 2), (8, 2), (4, 1)}))
    assert int(desc["m"][3 * 3 + 2]) == 0
    exprs = C2_LIKE + [Q.FieldToken("level", "absent-level-0"), Q.And(Q.FieldToken("service", "absent-svc-1"), Q.Token("absent-token"))]
    want = check_routes(ctx, [(words, desc)], exprs)
    assert (int(want[0][len(C2_LIKE), 0]) >> 3) & 1 and (int(want[0][len(C2_LIKE), 0]) >> 8) & 1     # nil => cannot disqualify


def test_grouped_call_over_three_arenas(ctx):
    check_routes(ctx, [arena(ctx, 5, first=200), arena(ctx, 64), arena(ctx, 9)], C2_LIKE)


def test_130_arenas_take_the_device_memory_table(ctx):
    assert 130 > 128                                          # more records than the kernel arguments hold
    two = [arena(ctx, 2, first=2 * i) for i in range(4)]
    check_routes(ctx, [two[i % 4] for i in range(130)], C2_LIKE[:40])


def test_filter_beyond_2_31_bits(ctx):
    """one block whose token filter has m = 2^31 + 12 345 bits: the gather kernel's 64-bit modulo and 64-bit word index"""
    m, k = (1 << 31) + 12345, 10
    toks = ["tok%d" % i for i in range(3000)]
    sets = (["msg"], toks, ["msg::" + t for t in toks[:50]])
    desc = np.zeros(3, dtype=DESC_DTYPE)
    entries, fstart, cursor = [], [0], 0
    for c, s in enumerate(sets):
        mm, kk = (m, k) if c == 1 else O.estimate_parameters(len(s), 0.001)
        desc[c] = (cursor, mm, kk, 0)
        cursor += ((mm + 63) // 64 + 15) // 16 * 16
        entries += s
        fstart.append(len(entries))
    blob, off = pack_entries(entries)
    words = ctx.build(blob, off, np.asarray(fstart, dtype=np.uint32), desc, cursor)
    exprs = [Q.Token(t) for t in toks[:20]] + [Q.Token("absent%d" % i) for i in range(40)] + [Q.And(Q.Token(toks[7]), Q.Token(toks[2999])), None]
    want = check_routes(ctx, [(words, desc)], exprs)
    assert [int(x) for x in want[0][:20, 0]] == [1] * 20 and not want[0][20:60].all()


def test_async_and_survivor_rows(ctx):
    arenas = [arena(ctx, 65), arena(ctx, 9)]
    G = [2, 1]

    def run_async(aids, bid, nq, n_blocks):
        out = ctx.pinned_array(nq * sum(G) * 8).view(np.uint64)
        try:
            out[:] = 0
            ctx.probe_many_into(aids, bid, out, _lib.PROBE_ASYNC)
            ctx.sync()
            return [out[: nq * 2].reshape(nq, 2).copy(), out[nq * 2:].reshape(nq, 1).copy()]
        finally:
            ctx.pinned_free(out.view(np.uint8))

    def run_rows(aids, bid, nq, n_blocks):
        rows = ctx.pinned_array(nq * sum(G) * 8).view(np.uint64)
        hdr = ctx.pinned_array(nq * 2 * 4).view(np.uint32)
        try:
            ctx.probe_many_rows(aids, bid, rows, hdr)
            return [rows_to_dense(hdr[:nq], rows[: nq * 2], 65), rows_to_dense(hdr[nq:], rows[nq * 2:], 9)]
        finally:
            ctx.pinned_free(rows.view(np.uint8))
            ctx.pinned_free(hdr.view(np.uint8))

    check_routes(ctx, arenas, C2_LIKE, run_async)
    check_routes(ctx, arenas, C2_LIKE, run_rows)
