"""bsg_match_rows_wide_range / bsg_match_rows_wide_range_rows (k_match_rows_store_range / _tok / _gram): any number of queries over one
table that holds FieldRange conditions.  Every listed pair's bit row is compared with the single call for its query on the set's rows
(bsg_match_rows_range, itself checked against the Fraction restatement in its own file) and with the host matchers
(bsh_match_row_range AND bsh_match_row_with); the tagged lists with the bit rows.  A range condition listens only on rows of a set
that lists a query which uses it: that gate, and its deliberate difference from bsg_match_rows_many_range, has a test of its own."""
import itertools
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID, BSG_E_UNSUPPORTED, KIND_FIELD, KIND_FIELD_RANGE, KIND_FIELD_TOKEN, KIND_TOKEN, OP_TERM, BloomGpuError, op
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from tests import range_restatement as RR
from tests import substring_restatement as SR

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)
N_SETS, SET_ROWS = 3, 100                       # 300 rows: two workgroups, every set cut in the middle of a wave
NIL = {"ExpressionType": "CONDITION", "Condition": None}
NONE, ALL, LIST, DENSE = 0, 1, 2, 3             # the tags of a pair's header (bits 30-31)
# four distinct conditions of kinds 0, 1 and 2 (the tokens have 3 runes: tokens under the trigram spec too) ...
BLOOMS = [None, Q.Token("all"), Q.FieldToken("lvl", "err"), Q.Or(Q.Field("x"), Q.Token("all")), Q.And(Q.FieldToken("lvl", "inf"), Q.Field("x"))]
# ... and eleven of kind 6 (two more inside the last tree): closed, open and absent bounds, and lo > hi
R_ID, R_LOW, R_LAT, R_ANY, R_NEVER = (Q.FieldRange("id", 10, 120), Q.FieldRange("id", None, 50, hi_open=True), Q.FieldRange("lat", 5, None, lo_open=True),
                                      Q.FieldRange("lat", None, None), Q.FieldRange("id", 200, 100))
R_X, R_X1, R_TAIL, R_POINT = (Q.FieldRange("x", 1, 3, lo_open=True, hi_open=True), Q.FieldRange("x", None, 1), Q.FieldRange("id", 290, None),
                              Q.FieldRange("id", 150, 150))
RANGES = [None, NIL, R_ID, R_LOW, R_LAT, R_ANY, R_NEVER, R_X, Q.RangeOr(R_ID, R_LAT), Q.RangeAnd(R_ID, R_LAT), Q.RangeOr(R_X1, R_TAIL),
          Q.RangeAnd(Q.RangeOr(R_X, R_POINT), NIL), R_POINT, Q.RangeAnd(Q.FieldRange("lat", None, 10, hi_open=True), Q.FieldRange("id", 30, None))]
QUERIES = list(itertools.product(BLOOMS, RANGES))                # 70 (bloom, range) pairs: more than the batched call takes
FIRST = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
LISTS = [list(range(len(QUERIES))), [], list(range(1, len(QUERIES), 3))]     # the middle set lists nothing


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([q for l in lists for q in l], dtype=np.uint32)


def row(**kv):
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


def make_rows():
    rows = []
    for i in range(N_SETS * SET_ROWS):
        d = {"id": i, "lat": (i * 7 % 40) / 2, "lvl": "err" if i % 4 == 0 else "inf", "msg": "all set" if i % 5 == 0 else "got one"}
        if i % 3 == 0:
            d["x"] = i % 5
        rows.append(row(**d))
    return rows


ROWS = make_rows()


def host_bits(rows, bloom, rng, tok):
    return np.array([Hst.match_row_range(rng, r) and (bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) for r in rows], dtype=bool)


def single_bits(ctx, rows, bloom, rng, tok=None, fallback=()):
    hits, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(bloom, rng), tok)
    assert list(fb) == list(fallback)
    return hits


def test_seventy_queries_share_fifteen_conditions():
    b = Q.CompiledWideRangeBatch(QUERIES)
    assert b.n_queries == 70 > 64 and len(b.kinds) == 15 <= 64
    assert {KIND_FIELD, KIND_TOKEN, KIND_FIELD_TOKEN, KIND_FIELD_RANGE} == set(b.kinds) and b.kinds.count(KIND_FIELD_RANGE) == 11
    with pytest.raises(ValueError):
        Q.CompiledRangeQueryBatch(QUERIES)                           # the batched call's batch holds 64


@pytest.mark.parametrize("walker", WALKERS)
def test_every_listed_pair_is_the_single_call_and_the_host_matchers(ctx, walker):
    tok = SR.WALKERS[walker]
    off, sq = csr(LISTS)
    batch = Q.CompiledWideRangeBatch(QUERIES)
    words, pwo, fb = ctx.match_rows_wide_range(ROWS, batch, FIRST, off, sq, tok)
    assert list(fb) == [] and len(pwo) == len(sq) + 1 and len(words) == len(sq) * 2
    # the references once, over all rows: the single call per query, the host matchers per distinct side
    single = [single_bits(ctx, ROWS, bloom, rng, tok) for bloom, rng in QUERIES]
    host_bloom = [np.array([b is None or Hst.match_row(b, r, SR.spec_of(tok)) for r in ROWS]) for b in BLOOMS]
    host_range = [np.array([Hst.match_row_range(g, r) for r in ROWS]) for g in RANGES]
    some, none = 0, 0
    for s in range(N_SETS):
        lo, hi = int(FIRST[s]), int(FIRST[s + 1])
        for p in range(int(off[s]), int(off[s + 1])):
            q = int(sq[p])
            got = wide_pair_bits(words, pwo, p, hi - lo)
            assert np.array_equal(got, single[q][lo:hi]), (s, q)
            assert np.array_equal(got, (host_bloom[q // len(RANGES)] & host_range[q % len(RANGES)])[lo:hi]), (s, q)
            some += bool(got.any())
            none += not got.any()
    assert some and none
    # the implicit set (no set table): every query on every row, pair for pair the listed call's
    every, epwo, efb = ctx.match_rows_wide_range(ROWS, batch, tokenizer=tok)
    assert list(efb) == [] and len(epwo) == len(QUERIES) + 1
    for q in range(len(QUERIES)):
        bits = wide_pair_bits(every, epwo, q, len(ROWS))
        assert np.array_equal(bits, single[q]), q
        for s in range(N_SETS):
            lo, hi = int(FIRST[s]), int(FIRST[s + 1])
            for p in range(int(off[s]), int(off[s + 1])):
                if int(sq[p]) == q:
                    assert np.array_equal(wide_pair_bits(words, pwo, p, hi - lo), bits[lo:hi]), (s, q)


@pytest.mark.parametrize("walker", WALKERS)
def test_set_boundaries_inside_the_first_wave(ctx, walker):
    tok = SR.WALKERS[walker]
    qs = [QUERIES[i] for i in (2, 17, 22, 38, 51, 69)]
    first = np.array([0, 10, 37, 64, 65, 130, 300], dtype=np.uint32)             # boundaries at rows 10 and 37
    lists = [[0, 1, 2, 3, 4, 5], [], [0, 2, 4], [5], [1, 3], [2, 3]]
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_range(ROWS, Q.CompiledWideRangeBatch(qs), first, off, sq, tok)
    assert list(fb) == []
    single = [single_bits(ctx, ROWS, bloom, rng, tok) for bloom, rng in qs]
    assert all(s.any() for s in single[:5])
    for s in range(len(lists)):
        lo, hi = int(first[s]), int(first[s + 1])
        for p in range(int(off[s]), int(off[s + 1])):
            assert np.array_equal(wide_pair_bits(words, pwo, p, hi - lo), single[int(sq[p])][lo:hi]), (s, int(sq[p]))


BIG = RR.BIG                                    # 40 digits
EDGE_LITERALS = ["9007199254740993", "5.000", "5.0001", "-0.0", "-0.5", "18446744073709551616", "-9223372036854775808", BIG, '"5"', "true", "null"]
EDGE_ROWS = [('{"v":%s}' % s).encode() for s in EDGE_LITERALS] + [b'{"a":1,"":2}']
# bounds that straddle each literal: (field, lo, hi, lo_open, hi_open)
EDGE_BOUNDS = [("v", 9007199254740993, 9007199254740993, False, False), ("v", 9007199254740992, 9007199254740993, False, True),
               ("v", 9007199254740993, 9007199254740994, True, False), ("v", 5, 5, False, False), ("v", 5, 6, True, False), ("v", 4, 5, False, True),
               ("v", 0, 0, False, False), ("v", -1, 0, False, True), ("v", None, 0, False, True), ("v", 0, None, True, False),
               ("v", RR.I64_MAX, None, True, False), ("v", None, RR.I64_MAX, False, False), ("v", RR.I64_MIN, RR.I64_MIN, False, False),
               ("v", RR.I64_MIN, None, True, False), ("v", None, RR.I64_MIN, False, True), ("v", None, None, False, False),
               ("a", 1, 1, False, False), ("a", 2, 2, False, False), ("a", 12, 12, False, False), ("a", None, None, False, False)]


@pytest.mark.parametrize("walker", WALKERS)
def test_exact_edge_literals(ctx, walker):
    tok = SR.WALKERS[walker]
    conds = [Q.FieldRange(f, lo, hi, lo_open=lo_o, hi_open=hi_o) for f, lo, hi, lo_o, hi_o in EDGE_BOUNDS]
    rows = EDGE_ROWS * 6                         # 72 rows: past one wave
    words, pwo, fb = ctx.match_rows_wide_range(rows, Q.CompiledWideRangeBatch([(None, c) for c in conds]), tokenizer=tok)
    assert list(fb) == []
    got = np.array([wide_pair_bits(words, pwo, q, len(rows)) for q in range(len(conds))])
    want = np.array([[Hst.match_row_range(c, r) for r in rows] for c in conds])
    assert np.array_equal(got, want), [(EDGE_BOUNDS[q], rows[r]) for q, r in zip(*np.nonzero(got != want))][:6]
    v = {s: i for i, s in enumerate(EDGE_LITERALS)}
    column = lambda s: [bool(b) for b in got[:16, v[s]]]
    # what the bounds above say about some of the literals, written out: no float64 round trip anywhere
    assert column("9007199254740993") == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1]
    assert column("5.000") == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1]
    assert column("5.0001") == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1]
    assert column("-0.0") == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1]
    assert column("-0.5") == [0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1]
    assert column("18446744073709551616") == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1]
    assert column("-9223372036854775808") == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1]
    assert column(BIG) == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1]
    for s in ('"5"', "true", "null"):
        assert not got[:, v[s]].any()
    assert [bool(b) for b in got[16:, len(EDGE_LITERALS)]] == [True, False, False, True]      # the pathless 2 is no part of a's 1


@pytest.mark.parametrize("walker", WALKERS)
def test_sixty_four_range_conditions_on_one_field_in_one_table(ctx, walker):
    """one parse of the leaf serves all 64: each condition gets its own bit"""
    tok = SR.WALKERS[walker]
    pairs = RR.BOUND_PAIRS[100:164]
    conds = [RR.field_range(Q, "v", lo, hi) for lo, hi in pairs]
    batch = Q.CompiledWideRangeBatch([(None, c) for c in conds])
    assert batch.kinds == [KIND_FIELD_RANGE] * 64
    rows = [('{"v":%s}' % s).encode() for s in RR.PLAIN_LITERALS] * 3
    values = [RR.exact(s) for s in RR.PLAIN_LITERALS] * 3
    assert len(rows) > 64
    words, pwo, fb = ctx.match_rows_wide_range(rows, batch, tokenizer=tok)
    assert list(fb) == []
    for c, (lo, hi) in enumerate(pairs):
        want = [RR.inside(v, lo, hi) for v in values]
        assert wide_pair_bits(words, pwo, c, len(rows)).tolist() == want, (lo, hi)
        assert want == [Hst.match_row_range(conds[c], r) for r in rows]


GATE_ROWS = [b'{"v":1e3}', b'{"v":5}', b'{"v":2E1,"w":1}', b'not json']
GATE_QUERIES = [(None, Q.FieldRange("v", 5, 7)), (None, Q.FieldRange("w", 1, 1))]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_range_condition_listens_only_for_a_set_that_lists_a_query_using_it(ctx, walker):
    tok = SR.WALKERS[walker]
    rows = GATE_ROWS * 4
    first = np.array([0, 4, 8, 12, 16], dtype=np.uint32)
    off, sq = csr([[1], [0], [], [0, 1]])
    words, pwo, fb = ctx.match_rows_wide_range(rows, Q.CompiledWideRangeBatch(GATE_QUERIES), first, off, sq, tok)
    # set 0 lists only the query on w: neither exponent literal on v hands its row back (the row that is no JSON does: the set is walked);
    # set 1 lists the query on v: both do; set 2 lists nothing and is never walked: not even the row that is no JSON comes back
    assert list(fb) == [3, 4, 6, 7, 12, 14, 15]
    bits = [wide_pair_bits(words, pwo, p, 4).tolist() for p in range(4)]
    assert bits == [[False, False, True, False], [False, True, False, False], [False, True, False, False], [False, False, False, False]]
    # (set 3, query on w: row 14 is a fallback row by the query on v, so its bit is 0 and the host decides it)
    assert [Hst.match_row_range(GATE_QUERIES[0][1], r) for r in GATE_ROWS] == [False, True, False, False]
    assert [Hst.match_row_range(GATE_QUERIES[1][1], r) for r in GATE_ROWS] == [False, False, True, False]
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_range_rows(rows, Q.CompiledWideRangeBatch(GATE_QUERIES), first, off, sq, tok)
    assert list(rfb) == list(fb)
    assert [pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], 4).tolist() for p in range(4)] == [[2], [1], [1], []]
    # the batched call over the same rows and masks: ANY range condition of the table listens on a walked row
    masks = np.array([0b10, 0b01, 0, 0b11], dtype=np.uint64)
    planes, mfb = ctx.match_rows_many_range(rows, Q.CompiledRangeQueryBatch(GATE_QUERIES), first, masks, tok)
    assert list(mfb) == [0, 2, 3, 4, 6, 7, 12, 14, 15]
    assert planes[0].tolist() == [False] * 4 + [False, True, False, False] + [False] * 4 + [False, True, False, False]


def test_the_batched_call_still_hands_back_what_its_own_suite_states(ctx):
    """tests/test_match_many_range_gpu.py::test_rows_of_a_set_with_mask_0_are_never_walked, its rows and its statement"""
    rows = [b'{"v":1e3}', b'{"v":5}', b'{"v":2E1,"w":1}', b'{"v":6}', b'not json', b'{"v":7e0}', b'{"v":7}']
    first, masks = np.array([0, 2, 5, 7], dtype=np.uint32), np.array([0b01, 0, 0b10], dtype=np.uint64)
    planes, fb = ctx.match_rows_many_range(rows, Q.CompiledRangeQueryBatch(GATE_QUERIES), first, masks)
    assert list(fb) == [0, 5]
    assert planes.tolist() == [[False, True, False, False, False, False, False], [False] * 7]
    # the wide call over the same sets: row 5's set lists only the query on w, and its exponent literal sits on v
    off, sq = csr([[0], [], [1]])
    words, pwo, wfb = ctx.match_rows_wide_range(rows, Q.CompiledWideRangeBatch(GATE_QUERIES), first, off, sq)
    assert list(wfb) == [0]
    assert wide_pair_bits(words, pwo, 0, 2).tolist() == [False, True] and wide_pair_bits(words, pwo, 1, 2).tolist() == [False, False]


ROWS_QUERIES = [(None, R_NEVER), (None, R_ANY), (None, Q.FieldRange("id", 10, 12)), (None, R_LOW), (Q.FieldToken("lvl", "err"), Q.FieldRange("id", 210, 212)),
                (None, Q.FieldRange("id", None, 250, hi_open=True))]


@pytest.mark.parametrize("walker", WALKERS)
def test_every_pairs_list_is_the_set_bits_of_its_bit_row(ctx, walker):
    tok = SR.WALKERS[walker]
    batch = Q.CompiledWideRangeBatch(ROWS_QUERIES)
    lists = [[0, 1, 2, 3], [], [1, 4, 5]]
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_range(ROWS, batch, FIRST, off, sq, tok)
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, tok)
    assert list(fb) == [] and list(rfb) == [] and len(hdr) == len(sq)
    tags = []
    for p in range(len(sq)):
        ids = pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], SET_ROWS)
        assert np.array_equal(ids, np.flatnonzero(wide_pair_bits(words, pwo, p, SET_ROWS))), p
        tags.append(int(hdr[p]) >> 30)
    # nothing, everything, three rows and half of set 0; everything, one row and half of set 2
    assert tags == [NONE, ALL, LIST, DENSE, ALL, LIST, DENSE]
    assert pair_rows_list(int(hdr[2]), payload[int(pair_off[2]): int(pair_off[3])], SET_ROWS).tolist() == [10, 11, 12]
    assert pair_rows_list(int(hdr[5]), payload[int(pair_off[5]): int(pair_off[6])], SET_ROWS).tolist() == [12]
    # the payload capacity, as bsg_match_rows_wide_rows: exactly the needed length is enough, one u32 less is BSG_E_INVALID naming both
    need = len(payload)
    assert need > 4
    exact = ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, tok, payload_cap=need)
    for a, b in zip(exact, (hdr, pair_off, payload, rfb)):
        assert np.array_equal(a, b)
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, tok, payload_cap=need - 1)
    assert e.value.code == BSG_E_INVALID and str(need) in str(e.value) and str(need - 1) in str(e.value)
    plain = Q.CompiledWideBatch([Q.Token("all"), None, Q.Field("x"), Q.FieldToken("lvl", "err"), None, Q.Field("x")])
    with pytest.raises(BloomGpuError) as e0:
        ctx.match_rows_wide_rows(ROWS, plain, FIRST, off, sq, tok, payload_cap=1)
    assert e0.value.code == e.value.code


@pytest.mark.parametrize("walker", WALKERS)
def test_a_table_without_a_range_condition_is_the_wide_calls(ctx, walker):
    tok = SR.WALKERS[walker]
    items = [Q.Token("all"), Q.FieldToken("lvl", "err"), None, Q.Or(Q.Field("x"), Q.Token("all")), Q.And(Q.FieldToken("lvl", "inf"), Q.Field("x"))]
    batch = Q.CompiledWideBatch(items)
    ranged = Q.CompiledWideRangeBatch([(b, None) for b in items])                  # And(bloom | TRUE, TRUE): no kind-6 condition either
    assert KIND_FIELD_RANGE not in batch.kinds and KIND_FIELD_RANGE not in ranged.kinds
    off, sq = csr([[0, 1, 2, 3, 4], [], [1, 3]])
    w0, pwo0, fb0 = ctx.match_rows_wide(ROWS, batch, FIRST, off, sq, tok)
    w1, pwo1, fb1 = ctx.match_rows_wide_range(ROWS, batch, FIRST, off, sq, tok)
    w2, pwo2, fb2 = ctx.match_rows_wide_range(ROWS, ranged, FIRST, off, sq, tok)
    assert list(fb0) == list(fb1) == list(fb2) == [] and np.array_equal(pwo0, pwo1) and w0.any()
    assert np.array_equal(w0, w1) and np.array_equal(w0, w2)
    r0 = ctx.match_rows_wide_rows(ROWS, batch, FIRST, off, sq, tok)
    r1 = ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, tok)
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b)
    # the wide, the wide substring and the lookup calls still refuse the kind
    one = Q.CompiledWideRangeBatch(QUERIES[:8])
    for call in (ctx.match_rows_wide, ctx.match_rows_wide_rows, ctx.match_rows_wide_substr, ctx.match_rows_wide_substr_rows, ctx.match_rows_lookup,
                 ctx.match_rows_lookup_rows):
        with pytest.raises(BloomGpuError) as e:
            call(ROWS, one, tokenizer=tok)
        assert e.value.code == BSG_E_INVALID and "unknown kind 6" in str(e.value)


class RawBatch:
    """a table and programs as given: (kind, field, entry) conditions, one TERM program per query"""

    def __init__(self, conds, n_queries=1):
        self.kinds = [k for k, _, _ in conds]
        self.fields = [f for _, f, _ in conds]
        self.tokens = [t for _, _, t in conds]
        self.prog_ops = [op(OP_TERM, q % len(conds)) for q in range(n_queries)]
        self.prog_off = list(range(n_queries + 1))
        self.n_queries = n_queries


def test_refusals_before_any_launch(ctx):
    entry = Q.range_entry({"Field": "id", "Lo": 1, "Hi": 2})
    assert len(entry) == 17
    before = int(ctx.device_calls().sum())
    for call in (ctx.match_rows_wide_range, ctx.match_rows_wide_range_rows):
        for kind, field, token in ((3, b"msg", b"a|b"), (4, b"", b"needle"), (5, b"msg", b"needle")):
            with pytest.raises(BloomGpuError) as e:
                call(ROWS[:10], RawBatch([(KIND_FIELD_RANGE, b"id", entry), (kind, field, token)]))
            assert e.value.code == BSG_E_UNSUPPORTED and "condition 1" in str(e.value) and "kind %d" % kind in str(e.value)
        with pytest.raises(BloomGpuError) as e:                       # 65 distinct conditions
            call(ROWS[:10], RawBatch([(KIND_FIELD_RANGE, b"id", Q.range_entry({"Field": "id", "Lo": c, "Hi": c})) for c in range(65)]))
        assert e.value.code == BSG_E_UNSUPPORTED and "65 conditions" in str(e.value)
        for bad in (entry[:16], entry + b"\0", entry[:16] + bytes([16])):        # 16 bytes, 18 bytes, a flag bit above 3
            with pytest.raises(BloomGpuError) as e:
                call(ROWS[:10], RawBatch([(KIND_TOKEN, b"", b"all"), (KIND_FIELD_RANGE, b"id", bad)]))
            assert e.value.code == BSG_E_INVALID and "condition 1" in str(e.value)
        with pytest.raises(BloomGpuError) as e:
            call(ROWS[:10], RawBatch([(7, b"id", entry)]))
        assert e.value.code == BSG_E_INVALID and "unknown kind 7" in str(e.value)
    assert int(ctx.device_calls().sum()) == before


def test_rows_that_travel_in_several_chunks_give_the_same_result(ctx):
    off, sq = csr(LISTS)
    batch = Q.CompiledWideRangeBatch(QUERIES)
    assert sum(len(r) for r in ROWS) > 3 * 4096
    one = ctx.match_rows_wide_range(ROWS, batch, FIRST, off, sq, SR.TRIGRAM)
    one_rows = ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, SR.TRIGRAM)
    try:
        ctx.set_ingest_chunk(4096)
        many = ctx.match_rows_wide_range(ROWS, batch, FIRST, off, sq, SR.TRIGRAM)
        many_rows = ctx.match_rows_wide_range_rows(ROWS, batch, FIRST, off, sq, SR.TRIGRAM)
    finally:
        ctx.set_ingest_chunk(0)
    for a, b in zip(one + one_rows, many + many_rows):
        assert np.array_equal(a, b)
    assert one[0].any()
