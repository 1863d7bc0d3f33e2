"""bsg_match_rows_wide_substr / bsg_match_rows_wide_substr_rows (k_match_rows_store_substr* / k_match_rows_store_regex_substr*): any number
of queries over one table that holds Substring / FieldSubstring conditions, with FieldRegex conditions beside them.  Every listed
pair's bit row is compared with the single call for its query on the set's rows (bsg_match_rows_substr / bsg_match_rows_regex_substr,
themselves checked against the restatements in their own files) and with the host matchers; the tagged lists with the bit rows."""
import itertools
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd._lib import KIND_FIELD, KIND_FIELD_SUBSTRING, KIND_FIELD_TOKEN, KIND_SUBSTRING, KIND_TOKEN
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from tests import substring_restatement as SR
from tests import test_match_many_regex_substr_gpu as RS
from tests.test_match_many_substr_gpu import MSGS
from tests.test_match_regex_substr_gpu import cap_rows, counted

pytestmark = pytest.mark.gpu

N_SETS, SET_ROWS = 3, 100                       # 300 rows: two workgroups, every set cut in the middle of a wave
NIL = {"ExpressionType": "CONDITION", "Condition": None}
# ten distinct conditions of kinds 0, 1, 2, 4 and 5 (the tokens have at most 3 runes: tokens under the trigram spec too); 32 needle bytes
BLOOMS = [None, Q.Token("all"), Q.FieldToken("lvl", "err"), Q.Or(Q.Field("x"), Q.Token("all")), Q.And(Q.FieldToken("lvl", "inf"), Q.Field("x"))]
NEEDLES = [Q.Substring("timeout"), Q.Substring("l go"), Q.FieldSubstring("msg", "conn"), Q.Substring("peer"), Q.FieldSubstring("x", "timeout 1"),
           Q.FieldSubstring("msg", "FULL")]
SUBS = [None, NIL] + NEEDLES + [Q.SubstringOr(NEEDLES[0], NEEDLES[2]), Q.SubstringAnd(NEEDLES[0], NEEDLES[2]), Q.SubstringOr(NEEDLES[1], NEEDLES[5], NEEDLES[3]),
                                Q.SubstringAnd(NEEDLES[3], NEEDLES[2]), Q.SubstringAnd(Q.SubstringOr(NEEDLES[4], NEEDLES[1]), NIL),
                                Q.SubstringOr(Q.SubstringAnd(NEEDLES[0], NEEDLES[4]), NEEDLES[5])]
QUERIES = list(itertools.product(BLOOMS, SUBS))                  # 70 (bloom, substring) pairs: more than any batched call takes
FIRST = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
LISTS = [list(range(len(QUERIES))), [], list(range(1, len(QUERIES), 3))]     # the middle set lists nothing


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.array([q for l in lists for q in l], dtype=np.uint32)


def batch_of(queries):
    return Q.CompiledWideSubstringBatch([(bloom, None, sub) for bloom, sub in queries])


def make_rows():
    """rows in the shape of tests/test_match_many_substr_gpu.py::make_rows"""
    rng = np.random.default_rng(5)
    rows = []
    for i in range(N_SETS * SET_ROWS):
        d = {"msg": MSGS[rng.integers(0, len(MSGS))], "lvl": ["err", "inf"][rng.integers(0, 2)]}
        if rng.random() < 0.3:
            d["x"] = "timeout %d" % i
        rows.append(json.dumps(d, separators=(",", ":")).encode())
    return rows


@pytest.fixture(scope="module")
def rows():
    return make_rows()


def test_seventy_queries_share_ten_conditions():
    b = batch_of(QUERIES)
    assert b.n_queries == 70 > 64 and len(b.kinds) == 10
    assert {KIND_FIELD, KIND_TOKEN, KIND_FIELD_TOKEN, KIND_SUBSTRING, KIND_FIELD_SUBSTRING} == set(b.kinds)
    with pytest.raises(ValueError):
        Q.CompiledRowSubstringQueryBatch([(bloom, None, sub) for bloom, sub in QUERIES])     # the batched call's batch holds 64


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_every_listed_pair_is_the_single_call_and_the_host_matchers(ctx, rows, walker):
    tok = SR.WALKERS[walker]
    off, sq = csr(LISTS)
    words, pwo, fb = ctx.match_rows_wide_substr(rows, batch_of(QUERIES), FIRST, off, sq, tok)
    assert list(fb) == [] and len(pwo) == len(sq) + 1 and len(words) == len(sq) * 2
    # the references once, over all rows: the single call per query, the host matchers per distinct side
    single = []
    for bloom, sub in QUERIES:
        hits, sfb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(bloom, sub), tok)
        assert list(sfb) == []
        single.append(hits)
    host_bloom = [np.array([b is None or Hst.match_row(b, r, SR.spec_of(tok)) for r in rows]) for b in BLOOMS]
    host_sub = [np.array([Hst.match_row_substring(s, r, tok) for r in rows]) for s in SUBS]
    some, none = 0, 0
    for s in range(N_SETS):
        lo, hi = int(FIRST[s]), int(FIRST[s + 1])
        for p in range(int(off[s]), int(off[s + 1])):
            q = int(sq[p])
            got = wide_pair_bits(words, pwo, p, hi - lo)
            assert np.array_equal(got, single[q][lo:hi]), (s, q)
            assert np.array_equal(got, (host_bloom[q // len(SUBS)] & host_sub[q % len(SUBS)])[lo:hi]), (s, q)
            some += bool(got.any())
            none += not got.any()
    assert some and none


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_kinds_0_to_5_in_one_table(ctx, walker):
    """the queries of the batched regex + substring suite: with a set table and as the implicit set"""
    tok = SR.WALKERS[walker]
    rows = RS.make_rows()
    batch = Q.CompiledWideSubstringBatch(RS.QUERIES)
    assert len(set(batch.kinds)) == 4 and set(batch.kinds) >= {3, 4, 5}
    first = np.arange(RS.N_SETS + 1, dtype=np.uint32) * RS.SET_ROWS
    lists = [[0, 1, 2, 3], [0, 2], [1, 3]]
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_substr(rows, batch, first, off, sq, tok)
    every, epwo, efb = ctx.match_rows_wide_substr(rows, batch, tokenizer=tok)
    assert list(fb) == [] and list(efb) == []
    single = []
    for bloom, rx, sx in RS.QUERIES:
        hits, sfb = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, rx, sx), tok)
        assert list(sfb) == [] and hits.any() and not hits.all()
        single.append(hits)
    for s in range(RS.N_SETS):
        lo, hi = int(first[s]), int(first[s + 1])
        for p in range(int(off[s]), int(off[s + 1])):
            assert np.array_equal(wide_pair_bits(words, pwo, p, hi - lo), single[int(sq[p])][lo:hi]), (s, int(sq[p]))
    for q in range(len(RS.QUERIES)):
        assert np.array_equal(wide_pair_bits(every, epwo, q, len(rows)), single[q]), q


def test_every_pairs_list_is_the_set_bits_of_its_bit_row(ctx, rows):
    off, sq = csr(LISTS)
    batch = batch_of(QUERIES)
    words, pwo, fb = ctx.match_rows_wide_substr(rows, batch, FIRST, off, sq)
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_substr_rows(rows, batch, FIRST, off, sq)
    assert list(fb) == [] and list(rfb) == [] and len(hdr) == len(sq)
    tags = set()
    for s in range(N_SETS):
        for p in range(int(off[s]), int(off[s + 1])):
            ids = pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], SET_ROWS)
            assert np.array_equal(ids, np.flatnonzero(wide_pair_bits(words, pwo, p, SET_ROWS))), p
            tags.add(int(hdr[p]) >> 30)
    assert {0, 2, 3} <= tags                     # NONE, LIST and DENSE pairs


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_a_needle_of_64_bytes_fills_the_first_word_and_the_next_starts_the_second(ctx, walker):
    tok = SR.WALKERS[walker]
    long_needle = "Needle-0123456789-ABCDEFGHIJKLMNOPQRSTUVWXYZ-0123456789-abcdefgh"
    assert len(SR.fold(long_needle, SR.spec_of(tok))) == 64
    a, b = Q.Substring(long_needle), Q.Substring("q")        # first-fit: a ends at bit 63 of word 0, b starts at bit 0 of word 1
    queries = [(None, a), (None, b), (None, Q.SubstringAnd(a, b)), (None, Q.SubstringOr(a, b)), (None, Q.SubstringAnd(b, a))]
    lower = long_needle.lower()
    rows = [('{"m":"xx %s yy"}' % lower).encode(), ('{"m":"xx %s yy"}' % lower[:-1]).encode(), ('{"m":"q %s"}' % lower).encode(),
            ('{"m":"%s","n":"Q"}' % long_needle[:-1]).encode(), b'{"m":"nothing"}', ('{"m":"%s%s"}' % (lower[:-1], lower)).encode()]
    rows = rows * 11                             # 66 rows: past one wave
    words, pwo, fb = ctx.match_rows_wide_substr(rows, batch_of(queries), tokenizer=tok)
    assert list(fb) == []
    for q, (_, sub) in enumerate(queries):
        host = np.array([Hst.match_row_substring(sub, r, tok) for r in rows])
        assert np.array_equal(wide_pair_bits(words, pwo, q, len(rows)), host), q
    first = wide_pair_bits(words, pwo, 0, len(rows))[:6].tolist()
    assert first == [True, False, True, False, False, True]
    # one more byte does not pack: refused before anything is launched
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_substr(rows, batch_of([(None, Q.SubstringAnd(a, b, Q.Substring(long_needle[::-1])))]), tokenizer=tok)
    assert "do not fit" in str(e.value)


# ten counted DFAs: 4 * (sum of the counts) + 2 820 bytes of blob (tests/test_match_regex_substr_gpu.py): 42 496 exactly, and 42 500 with one
# more state
AT_WIDE_SUB_CAP, OVER_WIDE_SUB_CAP = [991] * 9 + [1000], [991] * 8 + [992, 1000]


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_regex_tables_that_fill_the_cap_beside_the_needle_table(ctx, walker):
    """the blob takes every byte the needle table leaves of the 80 KiB (39 424 + 42 496): the last region and the field strings sit in
    the highest LDS bytes of the workgroup, and the last field's leaf is matched through them; one state more is refused before any launch"""
    tok = SR.WALKERS[walker]
    assert 4 * sum(AT_WIDE_SUB_CAP) + 2820 == 42496 == 80 * 1024 - 39424
    rows = cap_rows(AT_WIDE_SUB_CAP)
    needle = Q.FieldSubstring("z", "needle")
    batch = Q.CompiledWideSubstringBatch([(None, Q.RegexOr(*counted(AT_WIDE_SUB_CAP)), needle), (None, counted(AT_WIDE_SUB_CAP)[-1], None), (None, None, needle)])
    words, pwo, fb = ctx.match_rows_wide_substr(rows, batch, tokenizer=tok)
    assert list(fb) == []
    got = [wide_pair_bits(words, pwo, q, len(rows)).tolist() for q in range(3)]
    assert got == [[True, False, False, True, False], [True, False, False, False, False], [True, True, False, True, True]]
    over = Q.CompiledWideSubstringBatch([(None, Q.RegexOr(*counted(OVER_WIDE_SUB_CAP)), needle)])
    before = int(ctx.device_calls().sum())
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_substr(rows, over, tokenizer=tok)
    assert "LDS" in str(e.value) and "42496" in str(e.value) and int(ctx.device_calls().sum()) == before
    # without the needle the same tables are the wide call's, under its own cap
    plain = Q.CompiledWideSubstringBatch([(None, Q.RegexOr(*counted(OVER_WIDE_SUB_CAP)), None)])
    words, pwo, fb = ctx.match_rows_wide_substr(cap_rows(OVER_WIDE_SUB_CAP), plain, tokenizer=tok)
    assert list(fb) == [] and wide_pair_bits(words, pwo, 0, 5).tolist() == [True, False, True, True, False]


def test_rows_the_device_cannot_decide_are_handed_back_only_from_a_set_with_a_pair(ctx, rows):
    """the middle set holds a cut-off JSON row and a row with a rune the lower table does not know: with no pair listed on the set
    they are not walked and not reported; with one they are fallback rows and their pair bits are 0"""
    bad = list(rows)
    bad[SET_ROWS + 3] = b'{"msg":"connection re'
    bad[SET_ROWS + 9] = '{"msg":"connection \u0378 reset"}'.encode()
    batch = batch_of(QUERIES)
    off, sq = csr(LISTS)
    words, pwo, fb = ctx.match_rows_wide_substr(bad, batch, FIRST, off, sq)
    good, _, gfb = ctx.match_rows_wide_substr(rows, batch, FIRST, off, sq)
    assert list(fb) == [] and list(gfb) == [] and np.array_equal(words, good)
    lists = [LISTS[0], [4, 5], LISTS[2]]         # FieldSubstring(msg, conn) and Substring(peer) on the middle set
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_substr(bad, batch, FIRST, off, sq)
    good, _, _ = ctx.match_rows_wide_substr(rows, batch, FIRST, off, sq)
    assert list(fb) == [SET_ROWS + 3, SET_ROWS + 9]
    for p in range(int(off[1]), int(off[2])):
        got, ref = wide_pair_bits(words, pwo, p, SET_ROWS), wide_pair_bits(good, pwo, p, SET_ROWS)
        assert not got[[3, 9]].any()
        keep = np.ones(SET_ROWS, dtype=bool)
        keep[[3, 9]] = False
        assert np.array_equal(got[keep], ref[keep]) and got.any()
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_substr_rows(bad, batch, FIRST, off, sq)
    assert list(rfb) == [SET_ROWS + 3, SET_ROWS + 9]
    for p in range(len(sq)):
        ids = pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], SET_ROWS)
        assert np.array_equal(ids, np.flatnonzero(wide_pair_bits(words, pwo, p, SET_ROWS))), p


def test_rows_that_travel_in_several_chunks_give_the_same_result(ctx, rows):
    off, sq = csr(LISTS)
    batch = batch_of(QUERIES)
    assert sum(len(r) for r in rows) > 3 * 4096
    one = ctx.match_rows_wide_substr(rows, batch, FIRST, off, sq, SR.TRIGRAM)
    one_rows = ctx.match_rows_wide_substr_rows(rows, batch, FIRST, off, sq, SR.TRIGRAM)
    try:
        ctx.set_ingest_chunk(4096)
        many = ctx.match_rows_wide_substr(rows, batch, FIRST, off, sq, SR.TRIGRAM)
        many_rows = ctx.match_rows_wide_substr_rows(rows, batch, FIRST, off, sq, SR.TRIGRAM)
    finally:
        ctx.set_ingest_chunk(0)
    for a, b in zip(one + one_rows, many + many_rows):
        assert np.array_equal(a, b)
    assert one[0].any()


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_a_table_without_needles_is_the_wide_calls(ctx, rows, walker):
    """the same batch through both calls: a table with FieldRegex conditions, one with plain conditions only"""
    tok = SR.WALKERS[walker]
    items = [Q.Token("all"), (Q.FieldToken("lvl", "err"), Q.FieldRegex("msg", "timeout|conn")), (None, Q.FieldRegex("x", "^timeout 1")), None,
             Q.Or(Q.Field("x"), Q.Token("all"))]
    off, sq = csr([[0, 1, 2, 3, 4], [], [1, 2]])
    poff, psq = csr([[0, 1, 2], [], [2]])
    for batch, o, s in ((Q.CompiledWideBatch(items), off, sq), (Q.CompiledWideBatch([i for i in items if not isinstance(i, tuple)]), poff, psq)):
        assert not {KIND_SUBSTRING, KIND_FIELD_SUBSTRING} & set(batch.kinds)
        w0, pwo0, fb0 = ctx.match_rows_wide(rows, batch, FIRST, o, s, tok)
        w1, pwo1, fb1 = ctx.match_rows_wide_substr(rows, batch, FIRST, o, s, tok)
        assert list(fb0) == list(fb1) == [] and np.array_equal(pwo0, pwo1) and w0.any()
        assert np.array_equal(w0, w1)
        r0 = ctx.match_rows_wide_rows(rows, batch, FIRST, o, s, tok)
        r1 = ctx.match_rows_wide_substr_rows(rows, batch, FIRST, o, s, tok)
        for a, b in zip(r0, r1):
            assert np.array_equal(a, b)
    # the wide call itself still refuses the kinds
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide(rows, batch_of(QUERIES[:8]), tokenizer=tok)
    assert "unknown kind" in str(e.value)
