"""The gather kernels' order of a lane's locations (ascending 128-byte span of the filter, ties by hash index: csrc/kernels.hip.h,
restated in tests/gather_order_shapes.py).  Every case forces the gather with bsg_set_gather_cost(0) and compares the survivors bit
for bit with the tree-walking oracle and with the streamed route (bsg_set_gather_cost(1 << 20)); bsg_lab_last_probe_route names the
kernel family of each.  The filters are hand-sized (m, k) so that the shapes are those at which the order can go wrong: k of 1, 2, 4
(shorter than the phase list's prefix), 10, 16 (the sorted path's two widths) and 17 (index order); m of at most 1 024 bits (one span:
every key equal but for the index), 1 025 (two spans), a nil filter; a term with two equal locations; 1 / 29 / 64 / 65 terms; all
present, all absent and the C2 mix; arenas of 1, 7, 8, 9 and 65 blocks, two sizes in one call; 130 arenas through k_gather_fused.
The last test pins the ORDER: the executed bit tests the device counted equal the restatement's count."""
import math

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import DESC_DTYPE
from bloomsearch_amd.gpu import pack_entries
from oracle import oracle as O
from tests import gather_order_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

_arenas = {}


def ft(v, f="pair"):
    return Q.FieldToken(f, v)


def make_arena(n_blocks, m, k, n_values=60, first=0, nil=(), extra=()):
    """-> (words, desc), built by the oracle once per geometry: block b's field::token filter has m bits (m = None: sized for fpr 0.001)
    and k locations and holds pair::c0 .. c16 (in every block), pair::v<j> for n_values block-specific j, and `extra`; nil: blocks whose
    field::token filter is nil.  The field and token filters are one word each."""
    key = (n_blocks, m, k, n_values, first, tuple(nil), tuple(extra))
    if key not in _arenas:
        desc = np.zeros(3 * n_blocks, dtype=DESC_DTYPE)
        entries, fstart, cursor = [], [0], 0
        for b in range(n_blocks):
            vals = ["pair::c%d" % i for i in range(17)] + ["pair::v%d" % ((first + b) * n_values + j) for j in range(n_values)] + list(extra)
            mk = (m, k) if m is not None else O.estimate_parameters(len(vals), 0.001)
            for c, (mm, kk, s) in enumerate(((64, 1, ["pair"]), (64, 1, ["c0"]), (mk[0], mk[1], vals))):
                if c == 2 and b in nil:
                    fstart.append(len(entries))
                    continue
                desc[b * 3 + c] = (cursor, mm, kk, 0)
                cursor += ((mm + 63) // 64 + 1) // 2 * 2
                entries += s
                fstart.append(len(entries))
        blob, off = pack_entries(entries)
        _arenas[key] = (O.build_many(blob, off, np.asarray(fstart, dtype=np.uint32), desc.view(O.DESC_DTYPE), max(cursor, 2)), desc)
    return _arenas[key]


PRESENT = [ft("c%d" % i) for i in range(17)]
ABSENT = [ft("ghost%d" % i) for i in range(48)]
C2_MIX = PRESENT + ABSENT[:12]                                   # 29 terms: 17 in every block, 12 in none


def with_programs(terms):
    return terms + [Q.And(terms[0], terms[-1]), Q.Or(terms[len(terms) // 2], terms[-1]), Q.And(*terms[:3])]


def check(ctx, arenas, exprs, key27=1, route=_lib.ROUTE_GATHER):
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    nq = len(exprs)
    distinct = {id(w): (w, d) for w, d in arenas}
    want = {i: O.survivors_tree(w, d.view(O.DESC_DTYPE), exprs) for i, (w, d) in distinct.items()}
    loaded = {i: ctx.arena_load(w, d) for i, (w, d) in distinct.items()}
    aids = [loaded[id(w)] for w, _ in arenas]
    n_blocks = [len(d) // 3 for _, d in arenas]
    bid = ctx.batch_create(H.gpu_terms(ctx, cb), ops, poff)
    try:
        ctx.set_lab(3, 0)                                        # no one-dispatch path: the probe is a dispatch of its own
        ctx.set_lab(27, key27)
        ctx.set_gather_cost(0)
        got = ctx.probe_many(aids, bid, 0, nq, n_blocks)
        assert ctx.last_probe_route() == route, ctx.last_probe_route()
        ctx.set_gather_cost(1 << 20)
        streamed = ctx.probe_many(aids, bid, 0, nq, n_blocks)
        assert ctx.last_probe_route() == _lib.ROUTE_STREAM, ctx.last_probe_route()
        for i, (w, _) in enumerate(arenas):
            assert np.array_equal(got[i], want[id(w)]), "gathered survivors of arena %d differ from the tree-walking oracle" % i
            assert np.array_equal(got[i], streamed[i]), "gathered and streamed survivors of arena %d differ" % i
    finally:
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        for a in loaded.values():
            ctx.arena_free(a)
    return [want[id(w)] for w, _ in arenas]


@pytest.mark.parametrize("k", [1, 2, 4, 10, 16, 17])
@pytest.mark.parametrize("n_blocks", [1, 9])
def test_k_below_inside_and_beyond_the_sorted_widths(ctx, k, n_blocks):
    want = check(ctx, [make_arena(n_blocks, 20011, k)], with_programs(C2_MIX))
    assert [int(x) for x in want[0][:17, 0]] == [(1 << n_blocks) - 1] * 17


@pytest.mark.parametrize("m", [64, 700, 1024, 1025, 2048, 2049])
def test_filters_of_one_and_two_spans(ctx, m):
    """m <= 1 024: every location in span 0, the keys differ in the index alone; 1 025: one bit in span 1"""
    check(ctx, [make_arena(8, m, 10, n_values=3)], with_programs(C2_MIX))


def test_a_term_with_two_equal_locations(ctx):
    m, k = 1025, 10
    inside, i, j = S.a_word_with_two_equal_locations(m, k, prefix="pair::e")
    outside, _, _ = S.a_word_with_two_equal_locations(m, k, prefix="pair::g")
    words, desc = make_arena(7, m, k, n_values=3, extra=(inside,))
    exprs = with_programs([ft(inside[6:]), ft(outside[6:])] + C2_MIX)
    want = check(ctx, [(words, desc)], exprs)
    assert int(want[0][0, 0]) == 0x7F


def test_a_nil_filter_among_real_ones(ctx):
    words, desc = make_arena(9, None, None, nil=(3, 8))
    assert int(desc["m"][3 * 3 + 2]) == 0 and int(desc["k"][2]) == 10
    want = check(ctx, [(words, desc)], with_programs(C2_MIX))
    assert all((int(want[0][q, 0]) >> 3) & 1 and (int(want[0][q, 0]) >> 8) & 1 for q in range(29))          # nil => cannot disqualify
    assert not any(int(want[0][q, 0]) & 1 for q in range(17, 29))


@pytest.mark.parametrize("n_terms", [1, 29, 64, 65])
def test_term_counts(ctx, n_terms):
    """65: two term words, the second with one term and 63 padded lanes"""
    terms = (PRESENT + ABSENT)[:n_terms] if n_terms != 29 else C2_MIX
    check(ctx, [make_arena(65, None, None)], with_programs(terms))


@pytest.mark.parametrize("name,terms", [("all present", PRESENT), ("all absent", ABSENT[:29])])
def test_all_present_and_all_absent(ctx, name, terms):
    want = check(ctx, [make_arena(65, None, None)], with_programs(terms))
    passing = sum(bin(int(x)).count("1") for x in want[0][:len(terms)].ravel())
    # (all absent: the filters' false positives, 0.001 of 29 x 65 pairs in expectation, stay)
    assert passing == len(terms) * 65 if name == "all present" else passing < 20


def test_two_arenas_of_different_block_counts_in_one_call(ctx):
    check(ctx, [make_arena(7, None, None, first=100), make_arena(65, None, None), make_arena(8, 1025, 10, n_values=3)], with_programs(C2_MIX))


@pytest.mark.parametrize("key27,route", [(1, _lib.ROUTE_GATHER), (3, _lib.ROUTE_GATHER_CHUNKED)])
def test_130_arenas_through_both_gather_kernels(ctx, key27, route):
    """130 arena records lie in device memory (k_probe_gather_ext); in three chunks k_gather_fused runs the same role"""
    four = [make_arena(8, None, None, first=8 * i) for i in range(3)] + [make_arena(9, 20011, 16)]
    check(ctx, [four[i % 4] for i in range(130)], with_programs(C2_MIX), key27=key27, route=route)


def test_the_device_counts_the_tests_of_the_restated_order(ctx):
    """A timestamped launch sums the bit tests its lanes executed; bsg_timing.stream_bytes is bsh::gathered_bytes_tests of that sum:
    L (1 - exp(-t / L)) lines of 128 bytes per block, L the mean lines per filter, t the tests per block.  At this shape one test more
    or fewer moves the figure by tens of bytes, so the bytes (to the 2 that exp may differ by) name the count — and the count names the
    order: the restatement's index order executes another number of tests on this input (asserted first)."""
    n_blocks = 64
    words, desc = make_arena(n_blocks, None, None, n_values=20000)         # ~281 lines per filter against ~205 tests per block
    assert int(desc["k"][2]) == 10
    cb = Q.compile_queries(C2_MIX)
    ops, poff, kinds = cb.arrays()
    counts = {o: sum(x[0] for x in S.walk_arena(words, desc, cb.term_strings, [int(v) for v in kinds], o)) for o in ("index", "line")}
    assert counts["index"] != counts["line"], counts
    sum_words = sum((int(desc["m"][b * 3 + 2]) + 63) // 64 for b in range(n_blocks))
    lines = sum_words * 8 / 128 / n_blocks

    def model(tests):
        return lines * (1 - math.exp(-(tests / n_blocks) / lines)) * 128 * n_blocks

    assert model(counts[S.SHIPPED] + 1) - model(counts[S.SHIPPED]) > 16 and model(counts[S.SHIPPED]) < sum_words * 8
    other = "index" if S.SHIPPED == "line" else "line"
    assert abs(model(counts[other]) - model(counts[S.SHIPPED])) > 16
    aid = ctx.arena_load(words, desc)
    bid = ctx.batch_create(H.gpu_terms(ctx, cb), ops, poff)
    try:
        ctx.set_lab(3, 0)
        ctx.set_lab(27, 1)
        ctx.set_gather_cost(0)
        ctx.timing_read(reset=True)
        got = ctx.probe_many([aid], bid, _lib.PROBE_TIMED, len(C2_MIX), [n_blocks])
        assert ctx.last_probe_route() == _lib.ROUTE_GATHER
        t = ctx.timing_read(reset=True)
        assert t.n_probes == 1
        print("executed tests: restated index %d, line %d; stream_bytes %d, model(line) %.1f, model(index) %.1f"
              % (counts["index"], counts["line"], int(t.stream_bytes), model(counts["line"]), model(counts["index"])))
        assert np.array_equal(got[0], O.survivors_tree(words, desc.view(O.DESC_DTYPE), C2_MIX))
        assert abs(int(t.stream_bytes) - model(counts[S.SHIPPED])) <= 2, (int(t.stream_bytes), model(counts[S.SHIPPED]), counts)
    finally:
        ctx.set_lab(27, 0)
        ctx.set_gather_cost(_lib.GATHER_COST_DEFAULT)
        ctx.set_lab(3, 16)
        ctx.batch_free(bid)
        ctx.arena_free(aid)
