"""The gather kernels' phase schedule and their workgroups-per-CU cap (bsg_set_lab key 28: an LDS pad, bsh::gather_lds_pad) against the
oracle's probe_batch — never against another route of the library.  Every case runs under key 28 = 0 (the planner's rule), 1, 2 and 4
with bsg_set_gather_cost(0), and asserts that bsg_lab_last_probe_route names the gather kernel (the chunked route where key 27 forces
it: k_gather_fused under the pad).

The shapes are those at which the phases can go wrong: k = 1 .. 20 crosses and clips every phase boundary of every schedule the kernel
can be built with (lengths 1 .. 8, the last one repeating); terms that are present in some blocks and absent in others, and absent
terms whose first 1, 2, 3 and 4 locations are nevertheless set (found by searching strings with the oracle), so that a lane dies in
every phase while its neighbours go on; one term, a full term word, a padded second word; nil and tiny filters; partial workgroups
and verdict groups; records in the kernel arguments and in device memory.  Blocks of 200 rows as in test_probe_gather_gpu.py."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd.arena import entry_sets_from_strings, plan_blocks
from oracle import oracle as O
from tests import helpers as H
from tests.test_probe_gather_gpu import C2_LIKE, arena, field_token_terms

pytestmark = pytest.mark.gpu

CAPS = (0, 1, 2, 4)
_want = {}


def check(ctx, arenas, exprs, caps=CAPS, key27=None, tag=None):
    """arenas: [(words, desc)] -> the oracle's survivors per arena; the library's under every cap must equal them."""
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    terms = H.gpu_terms(ctx, cb)
    nq = len(exprs)
    want = []
    for w, d in arenas:
        key = (id(w), tag if tag is not None else id(exprs))
        if key not in _want:
            _want[key] = (w, exprs, O.probe_batch(w, d.view(O.DESC_DTYPE), terms.view(O.TERM_DTYPE), ops, poff))
        want.append(_want[key][2])
    n_blocks = [len(d) // 3 for _, d in arenas]
    loaded = {}
    for w, d in arenas:
        if id(w) not in loaded:
            loaded[id(w)] = ctx.arena_load(w, d)
    aids = [loaded[id(w)] for w, _ in arenas]
    bid = ctx.batch_create(terms, ops, poff)
    try:
        ctx.set_lab(3, 0)                                     # no one-dispatch path: the probe is a dispatch of its own
        ctx.set_gather_cost(0)
        ctx.set_lab(27, 1 if key27 is None else key27)
        for cap in caps:
            ctx.set_lab(28, cap)
            got = ctx.probe_many(aids, bid, 0, nq, n_blocks)
            assert ctx.last_probe_route() == (_lib.ROUTE_GATHER if key27 is None else _lib.ROUTE_GATHER_CHUNKED), (cap, ctx.last_probe_route())
            for i in range(len(arenas)):
                assert np.array_equal(got[i], want[i]), "key 28 = %d: gathered survivors of arena %d differ from the oracle" % (cap, i)
    finally:
        ctx.set_lab(28, 0)
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        for a in loaded.values():
            ctx.arena_free(a)
    return want


@pytest.mark.parametrize("n_blocks", [1, 7, 9, 65, 130])
def test_block_counts(ctx, n_blocks):
    want = check(ctx, [arena(ctx, n_blocks)], C2_LIKE, tag="c2")
    assert want[0].any() and not want[0].all()               # the batch prunes some (query, block) pairs and keeps others


@pytest.mark.parametrize("fpr,k", [(0.7, 1), (0.3, 2), (0.15, 3), (0.08, 4), (0.04, 5), (0.01, 7), (0.001, 10), (1e-6, 20)])
def test_k_across_every_phase_boundary(ctx, fpr, k):
    words, desc = arena(ctx, 9, fpr=fpr)
    assert int(desc["k"][2]) == k                             # (block 0's field::token filter)
    want = check(ctx, [(words, desc)], C2_LIKE, tag="c2")
    assert want[0].any()


@pytest.mark.parametrize("n_terms", [1, 29, 64, 65])
def test_term_counts(ctx, n_terms):
    terms = field_token_terms(n_terms)
    exprs = terms + [Q.And(terms[0], terms[-1]), Q.Or(terms[n_terms // 2], terms[-1])]
    check(ctx, [arena(ctx, 65)], exprs)


def test_a_nil_filter_among_real_ones(ctx):
    words, desc = arena(ctx, 9, absent=frozenset({(3, 2), (8, 2), (4, 1)}))
    assert int(desc["m"][3 * 3 + 2]) == 0
    exprs = C2_LIKE + [Q.FieldToken("level", "absent-level-0")]
    want = check(ctx, [(words, desc)], exprs)
    assert (int(want[0][len(C2_LIKE), 0]) >> 3) & 1 and (int(want[0][len(C2_LIKE), 0]) >> 8) & 1     # nil => cannot disqualify


def test_filters_of_a_few_words(ctx):
    words, desc = arena(ctx, 65, rows=3)
    assert int(desc["m"][2::3].max()) < 64 * 64
    check(ctx, [(words, desc)], C2_LIKE, tag="c2")


def term_string(expr):
    return Q.compile_queries([expr]).term_strings[0]


def hand_made_arena(ctx):
    """2 + 2 blocks of hand-made entry sets: the even blocks hold the field::token entries pair::v0 .. v119, the odd ones odd::v0 .. v119"""
    blocks = []
    for b in range(4):
        f = "pair" if b % 2 == 0 else "odd"
        vals = ["v%d" % i for i in range(120)]
        fts = [term_string(Q.FieldToken(f, v)) for v in vals]
        fts = [s.decode() if isinstance(s, bytes) else s for s in fts]
        blocks.append(entry_sets_from_strings([f], vals, fts))
    plan = plan_blocks(blocks, 0.001)
    return ctx.build(plan.blob, plan.off, plan.fstart, plan.desc, plan.n_words), plan.desc


def set_prefix(words, d, s):
    """how many of the string's first locations are set in filter d, stopping at the first that is not (k: all of them)"""
    h = O.base_hashes(s if isinstance(s, bytes) else s.encode())
    for i in range(int(d["k"])):
        loc = O.location(h, i) % int(d["m"])
        if not (int(words[int(d["word_off"]) + (loc >> 6)]) >> (loc & 63)) & 1:
            return i
    return int(d["k"])


def test_terms_that_die_in_every_phase(ctx):
    words, desc = hand_made_arena(ctx)
    k = int(desc["k"][3 + 2])
    assert k >= 8
    # present in the even blocks, absent from the odd ones — and the other way round
    exprs = [Q.FieldToken("pair", "v%d" % i) for i in range(6)] + [Q.FieldToken("odd", "v%d" % i) for i in range(6)]
    # absent from block 1, but its first 1 / 2 / 3 / 4 locations are set there: the lane goes on for that long and no longer
    found = {}
    for i in range(20000):
        e = Q.FieldToken("ghost", "g%d" % i)
        n = set_prefix(words, desc[3 + 2], term_string(e))
        if 1 <= n <= 4 and n not in found:
            found[n] = e
            if len(found) == 4:
                break
    assert sorted(found) == [1, 2, 3, 4]
    exprs += [found[n] for n in (1, 2, 3, 4)]
    exprs += [Q.And(exprs[0], found[4]), Q.Or(exprs[7], found[1]), Q.And(exprs[0], exprs[1])]
    want = check(ctx, [(words, desc)], exprs)
    assert [int(x) for x in want[0][:6, 0]] == [0b0101] * 6 and [int(x) for x in want[0][6:12, 0]] == [0b1010] * 6
    assert all(not (int(want[0][12 + j, 0]) >> 1) & 1 for j in range(4))


def test_grouped_call_over_three_arenas(ctx):
    check(ctx, [arena(ctx, 5, first=200), arena(ctx, 64), arena(ctx, 9)], C2_LIKE, tag="c2")


def test_130_arenas_of_8_blocks_take_the_device_memory_table(ctx):
    eight = [arena(ctx, 8, first=8 * i) for i in range(4)]
    check(ctx, [eight[i % 4] for i in range(130)], C2_LIKE[:40], tag="c2-40")


def test_the_chunked_route_under_the_pad(ctx):
    """key 27 = 3 chunks on 6 arenas of 65 blocks: k_probe_gather_ext, then k_gather_fused twice — its dynamic LDS is the larger of an
    evaluation workgroup's and the pad"""
    group = [arena(ctx, 65, first=100 * i) for i in range(6)]
    check(ctx, group, C2_LIKE, caps=(0, 2), key27=3, tag="c2")


def test_a_timed_launch_reports_the_lines_of_the_tests_it_executed(ctx):
    """bsg_timing.stream_bytes of a gathered launch is formed from the bit tests the kernel executed, counted on the device: terms
    present in every block run all k (the figure equals bsh::gathered_bytes' model of terms x k tests); an absent term runs at least
    up to its first clear bit and at most k, whatever the schedule — so the bytes lie between the model at those two test counts, and
    below the all-k figure.  The model: L (1 - exp(-t / L)) lines of 128 bytes per block, L the mean lines per filter."""
    import math
    assert term_string(Q.FieldToken("pair", "v1")) == b"pair::v1"
    vals = ["v%d" % i for i in range(20000)]                  # filters of ~280 lines: far more lines than tests, so the model tells the counts apart
    plan = plan_blocks([entry_sets_from_strings(["pair"], vals, ["pair::" + v for v in vals]) for b in range(4)], 0.001)
    words, desc = ctx.build(plan.blob, plan.off, plan.fstart, plan.desc, plan.n_words), plan.desc
    n_blocks = 4
    k = int(desc["k"][2])
    sum_words = sum((int(desc["m"][b * 3 + 2]) + 63) // 64 for b in range(n_blocks))
    lines = sum_words * 8 / 128 / n_blocks

    def model(tests_total):
        return min(lines * (1 - math.exp(-(tests_total / n_blocks) / lines)) * 128 * n_blocks, sum_words * 8)

    present = [Q.FieldToken("pair", "v%d" % i) for i in range(6)]
    ghosts = [Q.FieldToken("ghost", "g%d" % i) for i in range(6)]
    prefix = [[set_prefix(words, desc[b * 3 + 2], term_string(e)) for b in range(n_blocks)] for e in ghosts]
    assert all(p < k for row in prefix for p in row)          # absent everywhere, no false positive among them
    aid = ctx.arena_load(words, desc)
    try:
        ctx.set_lab(3, 0)
        ctx.set_gather_cost(0)
        ctx.set_lab(27, 1)
        got = {}
        for name, exprs in (("present", present), ("mixed", present + ghosts)):
            cb = Q.compile_queries(exprs)
            ops, poff, _ = cb.arrays()
            bid = ctx.batch_create(H.gpu_terms(ctx, cb), ops, poff)
            ctx.timing_read(reset=True)
            ctx.probe_many([aid], bid, _lib.PROBE_TIMED, len(exprs), [n_blocks])
            assert ctx.last_probe_route() == _lib.ROUTE_GATHER
            t = ctx.timing_read(reset=True)
            assert t.n_probes == 1
            got[name] = int(t.stream_bytes)
            ctx.batch_free(bid)
        all_k = 6 * k * n_blocks
        assert abs(got["present"] - model(all_k)) <= 2, (got, model(all_k))
        least = all_k + sum(p + 1 for row in prefix for p in row)
        assert model(least) - 2 <= got["mixed"] <= model(2 * all_k) + 2, (got, model(least), model(2 * all_k))
        assert got["mixed"] < model(2 * all_k) - 128          # the ghosts did not run all k: at least a line's worth fewer bytes
    finally:
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.arena_free(aid)
