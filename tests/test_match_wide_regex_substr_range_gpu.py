"""bsg_match_rows_wide_regex_substr_range / bsg_match_rows_wide_regex_substr_range_rows (k_match_rows_store_regex_substr_range / _tok /
_gram): any number of queries over ONE table that holds FieldRange conditions beside FieldRegex and substring ones.  Every listed
pair's bit row is compared with the restatements (tests/range_text_cases.want, which never ask the library) and with the single call
bsg_match_rows_regex_substr_range for its query on the set's rows; the tagged lists with the bit rows.  Regex and range conditions are
gated by the set's queries, needles are not: both gates, and their difference from the batched call, have tests of their own."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID, BSG_E_UNSUPPORTED, KIND_FIELD_RANGE, KIND_FIELD_REGEX, KIND_FIELD_SUBSTRING, KIND_SUBSTRING, KIND_TOKEN, BloomGpuError
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests import walker_envelope_shapes as WE
from tests.range_text_cases import AND, OR, T, row, want
from tests.test_match_many_regex_substr_range_gpu import FIRST, ROWS, make_rows
from tests.test_match_regex_substr_gpu import counted
from tests.test_match_regex_substr_range_gpu import cap_rows, host_verdict
from tests.test_match_wide_range_gpu import RawBatch, csr
from tests.test_match_wide_substr_gpu import AT_WIDE_SUB_CAP, OVER_WIDE_SUB_CAP
from tests.test_wide_range_text_cabi import QUERIES

pytestmark = pytest.mark.gpu

WALKERS = RT.WALKERS
NONE, ALL, LIST, DENSE = 0, 1, 2, 3             # the tags of a pair's header (bits 30-31)
LISTS = [list(range(len(QUERIES))), [], [3, 21, 36, 42, 69]]     # set 0 lists all 70, set 1 none, set 2 five


class Programs:
    """a table as given and one public program per query"""

    def __init__(self, m, progs):
        self.kinds, self.fields, self.tokens = list(m.kinds), list(m.fields), list(m.tokens)
        self.prog_ops = [o for p in progs for o in p]
        self.prog_off = [0]
        for p in progs:
            self.prog_off.append(self.prog_off[-1] + len(p))
        self.n_queries = len(progs)


@pytest.fixture(scope="module")
def rows():
    return make_rows()


@pytest.fixture(scope="module")
def expected(rows):
    """want() of every query under every walker, computed once"""
    return {w: [want(rows, *q, SR.WALKERS[w]) for q in QUERIES] for w in WALKERS}


@pytest.fixture(scope="module")
def singles(ctx, rows):
    """bsg_match_rows_regex_substr_range for every query over all rows under every walker, asked once"""
    out = {}
    for w in WALKERS:
        out[w] = []
        for quad in QUERIES:
            hits, fb = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowTextRangeQuery(*quad), SR.WALKERS[w])
            assert list(fb) == []
            out[w].append(hits)
    return out


def pair_bits(words, pwo, first, off):
    """[(set, pair, its bits)] of a call's result"""
    out = []
    for s in range(len(first) - 1):
        for p in range(int(off[s]), int(off[s + 1])):
            out.append((s, p, wide_pair_bits(words, pwo, p, int(first[s + 1]) - int(first[s]))))
    return out


# ---- 1 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_every_listed_pair_is_the_restatement_and_the_single_call(ctx, rows, expected, singles, walker):
    tok = SR.WALKERS[walker]
    batch = Q.CompiledWideTextRangeBatch(QUERIES)
    assert batch.n_queries == 70 and {KIND_FIELD_REGEX, KIND_SUBSTRING, KIND_FIELD_SUBSTRING, KIND_FIELD_RANGE} <= set(batch.kinds)
    off, sq = csr(LISTS)
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, batch, FIRST, off, sq, tok)
    assert list(fb) == [] and len(pwo) == len(sq) + 1 and len(words) == len(sq)          # every set has one tile
    some = none = 0
    for s, p, got in pair_bits(words, pwo, FIRST, off):
        q, lo, hi = int(sq[p]), int(FIRST[s]), int(FIRST[s + 1])
        assert np.array_equal(got, expected[walker][q][lo:hi]), (s, q)
        assert np.array_equal(got, singles[walker][q][lo:hi]), (s, q)
        some += bool(got.any())
        none += not got.any()
    assert some and none and int(off[1]) == int(off[2])                                  # set 1 has no pair: all zero ...
    # ... and is never walked: rows no walker can decide in it are not handed back, and no bit moves
    bad = list(rows)
    bad[43] = b'{"msg":"connection re'
    bad[64] = ('{"msg":"connection %s reset"}' % RT.unassigned_rune()).encode()
    bad[99] = b'{"ts":17e8,"msg":"timeout"}'
    again, _, fb = ctx.match_rows_wide_regex_substr_range(bad, batch, FIRST, off, sq, tok)
    assert list(fb) == [] and np.array_equal(again, words)
    # the implicit set (no set table): every query on every row
    every, epwo, efb = ctx.match_rows_wide_regex_substr_range(rows, batch, tokenizer=tok)
    assert list(efb) == [] and len(epwo) == len(QUERIES) + 1
    for q in range(len(QUERIES)):
        assert np.array_equal(wide_pair_bits(every, epwo, q, ROWS), expected[walker][q]), q


# ---- 2 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_set_boundaries_inside_the_first_wave(ctx, rows, expected, walker):
    tok = SR.WALKERS[walker]
    idx = [7, 21, 36, 42, 53, 69]
    first = np.array([0, 1, 3, 64, 65, 140], dtype=np.uint32)                    # sets of 1, 2, 61, 1 and 75 rows
    lists = [[0, 1, 2, 3, 4, 5], [], [0, 2, 4], [5], [1, 3]]
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch([QUERIES[i] for i in idx]), first, off, sq, tok)
    assert list(fb) == []
    seen = 0
    for s, p, got in pair_bits(words, pwo, first, off):
        assert np.array_equal(got, expected[walker][idx[int(sq[p])]][int(first[s]): int(first[s + 1])]), (s, int(sq[p]))
        seen += int(got.sum())
    assert seen > 0


# ---- 3 ----
@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("edge", range(len(RT.EDGES)), ids=[e[0].split(":")[0].replace(" ", "_")[:48] for e in RT.EDGES])
def test_edges_state_their_bits_through_the_implicit_set(ctx, walker, edge):
    tok = SR.WALKERS[walker]
    _, rows, rxs, sxs, rgs, progs = RT.EDGES[edge]
    m, _ = RT.table(rxs, sxs, rgs)
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Programs(m, [p for p, _ in progs]), tokenizer=tok)
    assert list(fb) == []
    for q, (prog, bits) in enumerate(progs):
        assert wide_pair_bits(words, pwo, q, len(rows)).tolist() == [bool(b) for b in bits], prog


# ---- 4 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_the_sixty_four_condition_table(ctx, walker):
    """16 tokens, 16 regex conditions, 16 needles filling both needle words, 16 ranges: one query per condition, bit 63 included, and an
    AND-of-four and an OR-of-four per side"""
    tok = SR.WALKERS[walker]
    rows, blooms, regexes, subs, ranges = RT.full_table()
    m, sides = RT.table(regexes, subs, ranges, blooms)
    assert len(m.kinds) == 64 and m.kinds[63] == KIND_FIELD_RANGE and sum(len(t) for t, k in zip(m.tokens, m.kinds) if k in (4, 5)) == 128
    sat = RT.sat_columns(rows, sides, tok)
    progs = [[T(c)] for c in range(64)]
    for side in range(4):
        four = [T(16 * side + j) for j in (0, 5, 10, 15)]
        progs += [four + [AND(4)], four + [OR(4)]]
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Programs(m, progs), tokenizer=tok)
    assert list(fb) == []
    for q, prog in enumerate(progs):
        got = wide_pair_bits(words, pwo, q, len(rows))
        assert np.array_equal(got, RT.evaluate(prog, sat)), q
        if q < 64:
            assert 0 < got.sum() < len(rows), q
    assert any(wide_pair_bits(words, pwo, q, len(rows)).any() for q in range(65, 72, 2))


# ---- 5 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_a_regex_condition_counts_only_where_the_set_lists_its_query(ctx, walker):
    """query 0 puts four regex conditions on the leaf `a`, query 1 a fifth: a row is handed back only in the set that lists both"""
    tok = SR.WALKERS[walker]
    queries = [(None, Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^err", "a", ".")]), Q.Substring("needle"), Q.FieldRange("n", 1, 9)),
               (None, Q.FieldRegex("a", "timeout|cache"), Q.Substring("x n"), Q.FieldRange("n", 5, None)),
               (None, None, Q.FieldSubstring("a", "NEEDLE"), Q.FieldRange("n", None, 5))]
    rows = [b'{"a":"err: x and a needle","n":3}', b'{"b":"x needle","n":5}', b'{"a":"cache x needle","n":7}'] * 2
    first = np.array([0, 3, 6], dtype=np.uint32)
    off, sq = csr([[0, 2], [0, 1, 2]])
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch(queries), first, off, sq, tok)
    assert list(fb) == [3, 5]
    w = [want(rows, *q, tok) for q in queries]
    assert w[0].tolist() == [True, False, False] * 2 and w[1].tolist() == [False, False, True] * 2 and w[2].tolist() == [True, False, False] * 2
    decided = np.array([True, True, True, False, True, False])
    for s, p, got in pair_bits(words, pwo, first, off):
        lo, hi = int(first[s]), int(first[s + 1])
        assert np.array_equal(got, (w[int(sq[p])] & decided)[lo:hi]), (s, int(sq[p]))


@pytest.mark.parametrize("walker", WALKERS)
def test_an_exponent_literal_hands_its_row_back_only_where_the_set_lists_a_query_on_its_field(ctx, walker):
    """the same input through both calls: the wide call asks the range conditions of the SET's queries, the batched call ANY of the table"""
    tok = SR.WALKERS[walker]
    queries = [(None, Q.FieldRegex("m", "timeout"), None, Q.FieldRange("v", 1000, 1000)), (None, None, Q.Substring("timeout"), Q.FieldRange("u", 1, 1))]
    rows = [b'{"v":1e3,"u":1,"m":"timeout"}', b'{"v":1000,"u":1,"m":"timeout"}', b'{"w":1e3,"v":1000,"u":2,"m":"timeout"}'] * 2
    first = np.array([0, 3, 6], dtype=np.uint32)
    off, sq = csr([[1], [0]])                                   # set 0: only the query on u; set 1: the query on v
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch(queries), first, off, sq, tok)
    assert list(fb) == [3]
    w = [want(rows, *q, tok) for q in queries]
    assert w[0].tolist() == [True, True, True] * 2 and w[1].tolist() == [True, True, False] * 2
    assert wide_pair_bits(words, pwo, 0, 3).tolist() == [True, True, False] == w[1][:3].tolist()     # {"v":1e3,...} is DECIDED here
    assert wide_pair_bits(words, pwo, 1, 3).tolist() == [False, True, True]                           # ... and handed back here
    planes, mfb = ctx.match_rows_many_regex_substr_range(rows, Q.CompiledRowTextRangeQueryBatch(queries), first, np.array([0b10, 0b01], dtype=np.uint64), tok)
    assert list(mfb) == [0, 3]
    assert planes[1].tolist() == [False, True, False] + [False] * 3 and planes[0].tolist() == [False] * 3 + [False, True, True]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_needle_no_listed_query_uses_changes_no_pair_bit(ctx, walker):
    tok = SR.WALKERS[walker]
    q0 = (None, Q.FieldRegex("m", "timeout"), Q.Substring("out"), Q.FieldRange("v", 5, 9))
    q1 = (None, None, Q.FieldSubstring("m", "timeout after"), Q.FieldRange("v", 7, None))
    rows = [row(m="timeout after 3 tries" if i % 2 else "time is out", v=i % 12) for i in range(70)]
    first = np.array([0, 30, 70], dtype=np.uint32)
    off, sq = csr([[0], [0, 1]])
    both, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch([q0, q1]), first, off, sq, tok)
    assert list(fb) == []
    alone, apwo, afb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch([q0]), first, *csr([[0], [0]]), tok)
    assert list(afb) == []
    w0, w1 = want(rows, *q0, tok), want(rows, *q1, tok)
    assert np.array_equal(wide_pair_bits(both, pwo, 0, 30), wide_pair_bits(alone, apwo, 0, 30)) and np.array_equal(wide_pair_bits(both, pwo, 0, 30), w0[:30])
    assert np.array_equal(wide_pair_bits(both, pwo, 1, 40), w0[30:]) and np.array_equal(wide_pair_bits(both, pwo, 2, 40), w1[30:])
    assert w0.any() and w1.any() and not w0.all()


@pytest.mark.parametrize("walker", WALKERS)
def test_rows_no_walker_decides_in_a_set_without_a_pair_are_not_handed_back(ctx, walker):
    tok = SR.WALKERS[walker]
    q0 = (None, Q.FieldRegex("m", "timeout"), Q.Substring("timeout"), Q.FieldRange("v", 1000, 1000))
    good = b'{"m":"timeout","v":1000}'
    bad = [b'{"m":"timeout","v":10', RT.DEEP17, ('{"m":"time%sout","v":1000}' % RT.unassigned_rune()).encode()]
    assert not WE.in_envelope(RT.DEEP17)
    rows = [good] + bad + [good] + bad + [good]
    first = np.array([0, 1, 4, 5, 8, 9], dtype=np.uint32)
    off, sq = csr([[0], [], [0], [0], [0]])
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch([q0]), first, off, sq, tok)
    assert list(fb) == [5, 6, 7]                                 # the same three rows in the set with a pair are
    assert [b.tolist() for _, _, b in pair_bits(words, pwo, first, off)] == [[True], [True], [False, False, False], [True]]


# ---- 6 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_the_largest_blob_beside_a_range_condition(ctx, walker):
    """42 496 bytes of regex tables fill the workgroup's 80 KiB behind the needle table, with a needle in it and without one: the last
    field's leaf is matched through the highest LDS bytes; four bytes more are refused before any launch"""
    tok = SR.WALKERS[walker]
    assert 4 * sum(AT_WIDE_SUB_CAP) + 2820 == 42496 and 4 * sum(OVER_WIDE_SUB_CAP) + 2820 == 42500
    rows, rg = cap_rows(AT_WIDE_SUB_CAP), Q.FieldRange("n", 5, 5)
    at, over = Q.RegexOr(*counted(AT_WIDE_SUB_CAP)), Q.RegexOr(*counted(OVER_WIDE_SUB_CAP))
    for sx, bits in ((Q.FieldSubstring("z", "needle"), [1, 0, 0, 0, 0]), (None, [1, 0, 1, 0, 0])):
        queries = [(None, at, sx, rg), (None, counted(AT_WIDE_SUB_CAP)[-1], None, None), (None, None, sx, rg)]
        batch = Q.CompiledWideTextRangeBatch(queries)
        assert (KIND_FIELD_SUBSTRING in batch.kinds) == (sx is not None) and KIND_FIELD_RANGE in batch.kinds
        words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, batch, tokenizer=tok)
        assert list(fb) == []
        got = [wide_pair_bits(words, pwo, q, len(rows)) for q in range(3)]
        assert got[0].tolist() == [bool(b) for b in bits] and got[1].tolist() == [True, False, False, False, False]
        for q, quad in enumerate(queries):
            assert np.array_equal(got[q], want(rows, *quad, tok)), q
        before = int(ctx.device_calls().sum())
        with pytest.raises(BloomGpuError) as e:
            ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch([(None, over, sx, rg)]), tokenizer=tok)
        assert e.value.code == BSG_E_UNSUPPORTED and "LDS" in str(e.value) and "42496" in str(e.value)
        assert int(ctx.device_calls().sum()) == before


# ---- 7 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_a_table_without_one_family_is_the_parents_call(ctx, rows, walker):
    tok = SR.WALKERS[walker]
    off, sq = csr([[0, 1, 2, 3], [], [1, 3]])
    bad = list(rows)
    bad[5] = ('{"msg":"connection %s reset","ts":1700000005}' % RT.unassigned_rune()).encode()      # handed back by the needles
    bad[110] = b'{"ts":17000001e2,"msg":"cache miss: timeout","lvl":"err","lat":3}'               # ... and by a range condition on ts
    # no kind 6: bsg_match_rows_wide_substr's bits, lists and fallback rows
    text = Q.CompiledWideSubstringBatch([(q[0], q[1], q[2]) for q in (QUERIES[1], QUERIES[6], QUERIES[21], QUERIES[36])])
    assert KIND_FIELD_RANGE not in text.kinds and KIND_FIELD_REGEX in text.kinds and KIND_SUBSTRING in text.kinds
    a, b = ctx.match_rows_wide_regex_substr_range(bad, text, FIRST, off, sq, tok), ctx.match_rows_wide_substr(bad, text, FIRST, off, sq, tok)
    assert list(a[2]) == list(b[2]) and 5 in list(a[2]) and a[0].any()
    for x, y in zip(a + ctx.match_rows_wide_regex_substr_range_rows(bad, text, FIRST, off, sq, tok), b + ctx.match_rows_wide_substr_rows(bad, text, FIRST, off, sq, tok)):
        assert np.array_equal(x, y)
    # kind 6 and no text kind: bsg_match_rows_wide_range's
    ranged = Q.CompiledWideRangeBatch([(q[0], q[3]) for q in (QUERIES[0], QUERIES[5], QUERIES[20], QUERIES[35])])
    assert KIND_FIELD_RANGE in ranged.kinds and not {KIND_FIELD_REGEX, KIND_SUBSTRING, KIND_FIELD_SUBSTRING} & set(ranged.kinds)
    a, b = ctx.match_rows_wide_regex_substr_range(bad, ranged, FIRST, off, sq, tok), ctx.match_rows_wide_range(bad, ranged, FIRST, off, sq, tok)
    assert list(a[2]) == list(b[2]) and 110 in list(a[2]) and a[0].any()
    for x, y in zip(a + ctx.match_rows_wide_regex_substr_range_rows(bad, ranged, FIRST, off, sq, tok), b + ctx.match_rows_wide_range_rows(bad, ranged, FIRST, off, sq, tok)):
        assert np.array_equal(x, y)
    # a table past a parent's own cap is refused with the parent's message: 42 500 bytes beside a needle and no range condition
    over = Q.CompiledWideSubstringBatch([(None, Q.RegexOr(*counted(OVER_WIDE_SUB_CAP)), Q.Substring("needle"))])
    said = []
    before = int(ctx.device_calls().sum())
    for call in (ctx.match_rows_wide_substr, ctx.match_rows_wide_regex_substr_range, ctx.match_rows_wide_regex_substr_range_rows):
        with pytest.raises(BloomGpuError) as e:
            call(rows[:5], over, tokenizer=tok)
        assert e.value.code == BSG_E_UNSUPPORTED
        said.append(str(e.value))
    assert said[0] == said[1] == said[2] and "42496" in said[0] and int(ctx.device_calls().sum()) == before
    # ... and without the needle the same tables are the wide call's, under its own 46 592 bytes
    plain = Q.CompiledWideSubstringBatch([(None, Q.RegexOr(*counted(OVER_WIDE_SUB_CAP)), None)])
    crow = cap_rows(OVER_WIDE_SUB_CAP)
    a, b = ctx.match_rows_wide_regex_substr_range(crow, plain, tokenizer=tok), ctx.match_rows_wide(crow, plain, tokenizer=tok)
    assert np.array_equal(a[0], b[0]) and list(a[2]) == list(b[2]) == [] and wide_pair_bits(a[0], a[1], 0, 5).tolist() == [True, False, True, True, False]
    # the parents still keep the other family out
    mixed = Q.CompiledWideTextRangeBatch(QUERIES[:8])
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_range(rows, mixed, tokenizer=tok)
    assert e.value.code == BSG_E_UNSUPPORTED
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_substr(rows, mixed, tokenizer=tok)
    assert e.value.code == BSG_E_INVALID and "unknown kind 6" in str(e.value)


# ---- 8 ----
ALWAYS = Q.FieldRange("ts", 1700000000, None)
ROWS_QUERIES = [(None, Q.FieldRegex("ts", "^17"), Q.Substring("10."), Q.FieldRange("ts", 200, 100)),             # lo > hi: nothing
                (None, Q.FieldRegex("ts", "^17"), Q.Substring("10."), ALWAYS),                                    # everything
                (None, Q.FieldRegex("ts", "^17"), None, Q.FieldRange("ts", 1700000010, 1700000010)),              # one row of set 0
                (None, None, Q.FieldSubstring("lvl", "err"), ALWAYS),                                             # about half
                (None, Q.FieldRegex("lvl", "^inf"), Q.Substring(".3."), Q.FieldRange("ts", 1700000110, 1700000111))]


@pytest.mark.parametrize("walker", WALKERS)
def test_every_pairs_list_is_the_set_bits_of_its_bit_row(ctx, rows, walker):
    tok = SR.WALKERS[walker]
    batch = Q.CompiledWideTextRangeBatch(ROWS_QUERIES)
    bad = list(rows)
    bad[7] = RT.DEEP17                                           # a fallback row in a set with pairs: in no list
    lists = [[0, 1, 2, 3], [], [1, 3, 4]]
    off, sq = csr(lists)
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(bad, batch, FIRST, off, sq, tok)
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_regex_substr_range_rows(bad, batch, FIRST, off, sq, tok)
    assert list(fb) == list(rfb) == [7] and len(hdr) == len(sq)
    tags = []
    for s, p, bits in pair_bits(words, pwo, FIRST, off):
        ids = pair_rows_list(int(hdr[p]), payload[int(pair_off[p]): int(pair_off[p + 1])], len(bits))
        assert np.array_equal(ids, np.flatnonzero(bits)), p
        assert s != 0 or 7 not in ids.tolist()
        tags.append(int(hdr[p]) >> 30)
    # set 0 (40 rows, one of them handed back): nothing, all but the fallback row, one row, about half; set 2: everything, about half, one or two rows
    assert tags[:3] == [NONE, DENSE, LIST] and tags[3] == DENSE and tags[4] == ALL and {NONE, ALL, LIST, DENSE} == set(tags)
    assert pair_rows_list(int(hdr[2]), payload[int(pair_off[2]): int(pair_off[3])], 40).tolist() == [10]
    # the payload capacity, as bsg_match_rows_wide_rows documents: the needed length is enough, one u32 less is BSG_E_INVALID naming both
    need = len(payload)
    assert need > 2
    exact = ctx.match_rows_wide_regex_substr_range_rows(bad, batch, FIRST, off, sq, tok, payload_cap=need)
    for a, b in zip(exact, (hdr, pair_off, payload, rfb)):
        assert np.array_equal(a, b)
    with pytest.raises(BloomGpuError) as e:
        ctx.match_rows_wide_regex_substr_range_rows(bad, batch, FIRST, off, sq, tok, payload_cap=need - 1)
    assert e.value.code == BSG_E_INVALID and str(need) in str(e.value) and str(need - 1) in str(e.value)


# ---- 9 ----
@pytest.mark.parametrize("walker", WALKERS)
def test_the_fallback_rows_are_the_union_of_the_parents_rules(ctx, walker):
    """a truncated row, seventeen open containers, an unassigned rune, an exponent literal where a listed query's range condition listens
    and a leaf under five regex conditions (one row with two causes) in ONE call: each listed once, ascending, every pair bit 0, and
    the host matchers decide them as the restatements do"""
    tok = SR.WALKERS[walker]
    u = RT.unassigned_rune()
    five = Q.RegexOr(*[Q.FieldRegex("a", p) for p in ("x", "^x", "x$", "^x$", ".")])
    queries = [(None, Q.RegexOr(five, Q.FieldRegex("m", "timeout")), Q.Substring("timeout"), Q.FieldRange("v", 1000, 1000)),
               (None, Q.FieldRegex("m", "timeout"), None, Q.FieldRange("u", 1, 1))]
    rows = [b'{"m":"timeout","v":1000,"u":1}', b'{"m":"timeout","v":10', RT.DEEP17, ('{"m":"time%sout timeout","v":1000,"u":1}' % u).encode(),
            b'{"v":1e3,"m":"timeout","u":1}', b'{"a":"x","v":1e3,"m":"timeout","u":1}', b'{"a":"x","v":1000,"m":"timeout","u":2}', b'{"m":"fine","v":1000,"u":1}']
    handed_back = [1, 2, 3, 4, 5, 6]
    words, pwo, fb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch(queries), tokenizer=tok)
    assert list(fb) == handed_back
    hdr, pair_off, payload, rfb = ctx.match_rows_wide_regex_substr_range_rows(rows, Q.CompiledWideTextRangeBatch(queries), tokenizer=tok)
    assert list(rfb) == handed_back
    for q, quad in enumerate(queries):
        got = wide_pair_bits(words, pwo, q, len(rows))
        assert got.tolist() == [True] + [False] * 7
        assert pair_rows_list(int(hdr[q]), payload[int(pair_off[q]): int(pair_off[q + 1])], len(rows)).tolist() == [0]
        for i in handed_back:
            # (a row that is no JSON object matches nothing; the restatements only read rows that parse)
            assert host_verdict(rows[i], *quad, tok) == (False if i == 1 else bool(RT.verdict(rows[i], *quad, tok))), (q, rows[i])
    assert [host_verdict(rows[i], *queries[0], tok) for i in handed_back] == [False, False, True, True, True, True]
    assert [host_verdict(rows[i], *queries[1], tok) for i in handed_back] == [False, False, True, True, True, False]
    # the set that lists only the query on u: the exponent literal on v and the five conditions on `a` hand nothing back there
    again, apwo, afb = ctx.match_rows_wide_regex_substr_range(rows, Q.CompiledWideTextRangeBatch(queries), np.array([0, 8], dtype=np.uint32), *csr([[1]]), tok)
    assert list(afb) == [1, 2, 3]
    assert wide_pair_bits(again, apwo, 0, 8).tolist() == [True, False, False, False, True, True, False, False]


# ---- 10 ----
def test_rows_that_travel_in_several_chunks_give_the_same_result(ctx):
    rows = [row(id=i, pad="x" * 600, msg="upstream timeout" if i % 2 == 0 else "cache warm", peer="10.0.3.%d" % i if i % 5 == 0 else "10.1.3.%d" % i, ts=1700000000 + i)
            for i in range(330)]
    rows[100] = b'{"msg":"upstream time'
    rows[201] = b'{"ts":17000002e2,"msg":"upstream timeout","peer":"10.0.3.1"}'
    assert sum(len(r) for r in rows) > 3 * (1 << 16)             # 64 KiB, the smallest chunk: at least three of them
    queries = [(None, Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3."), Q.FieldRange("ts", 1700000100, 1700000250, lo_open=True)),
               (None, None, Q.FieldSubstring("msg", "cache"), Q.FieldRange("id", None, 50)), (None, Q.FieldRegex("peer", "^10\\.1"), None, Q.FieldRange("id", 300, None))]
    batch = Q.CompiledWideTextRangeBatch(queries)
    first = np.array([0, 110, 220, 330], dtype=np.uint32)
    off, sq = csr([[0, 1, 2], [0], [0, 2]])
    one = ctx.match_rows_wide_regex_substr_range(rows, batch, first, off, sq, SR.TRIGRAM)
    one_rows = ctx.match_rows_wide_regex_substr_range_rows(rows, batch, first, off, sq, SR.TRIGRAM)
    try:
        ctx.set_ingest_chunk(1)                                  # its smallest
        many = ctx.match_rows_wide_regex_substr_range(rows, batch, first, off, sq, SR.TRIGRAM)
        many_rows = ctx.match_rows_wide_regex_substr_range_rows(rows, batch, first, off, sq, SR.TRIGRAM)
    finally:
        ctx.set_ingest_chunk(0)
    for a, b in zip(one + one_rows, many + many_rows):
        assert np.array_equal(a, b)
    assert list(one[2]) == [100, 201] and one[0].any()
    w = want(rows[:100], *queries[0], SR.TRIGRAM)
    assert np.array_equal(wide_pair_bits(one[0], one[1], 0, 110)[:100], w)


# ---- 11 ----
def test_refusals_before_any_launch(ctx):
    entry = Q.range_entry({"Field": "id", "Lo": 1, "Hi": 2})
    assert len(entry) == 17
    rng, rows = (KIND_FIELD_RANGE, b"id", entry), [b'{"id":1,"m":"x"}'] * 10
    rx = lambda i: (KIND_FIELD_REGEX, b"m", b"x%d" % i)
    sub = lambda s: (KIND_SUBSTRING, b"", s)
    cases = [
        ([rng] + [sub(b"n%02d" % i) for i in range(64)], BSG_E_UNSUPPORTED, ("65 conditions",)),
        ([rng] + [rx(i) for i in range(17)], BSG_E_UNSUPPORTED, ("17 regex conditions",)),
        ([rng, sub(b"a" * 65)], BSG_E_UNSUPPORTED, ("condition 1", "65 bytes")),
        ([rng, sub(b"a" * 40), sub(b"b" * 40), sub(b"c" * 40)], BSG_E_UNSUPPORTED, ("needles", "do not fit")),
        ([rng, sub(b"abc"), (7, b"m", b"x")], BSG_E_INVALID, ("condition 2", "unknown kind 7")),
        ([sub(b"abc"), (KIND_FIELD_RANGE, b"id", entry[:16])], BSG_E_INVALID, ("condition 1", "17 bytes")),
        ([sub(b"abc"), (KIND_FIELD_RANGE, b"id", entry[:16] + bytes([16]))], BSG_E_INVALID, ("condition 1", "flags")),
        ([rng, sub(b"")], BSG_E_INVALID, ("condition 1", "needle")),
        ([rng, (KIND_FIELD_SUBSTRING, b"m", b"\xff\xfe")], BSG_E_INVALID, ("condition 1", "needle")),
        ([rng, (KIND_FIELD_REGEX, b"m", b"\\bx")], BSG_E_UNSUPPORTED, ("regex condition 1",)),
    ]
    before = int(ctx.device_calls().sum())
    for call in (ctx.match_rows_wide_regex_substr_range, ctx.match_rows_wide_regex_substr_range_rows):
        for conds, code, words in cases:
            with pytest.raises(BloomGpuError) as e:
                call(rows, RawBatch(conds))
            assert e.value.code == code and all(w in str(e.value) for w in words), (conds[:3], str(e.value))
        # a query list that is not strictly ascending
        with pytest.raises(BloomGpuError) as e:
            call(rows, RawBatch([rng, sub(b"abc"), (KIND_TOKEN, b"", b"x")], n_queries=3), np.array([0, 10], dtype=np.uint32), np.array([0, 3], dtype=np.uint32),
                 np.array([0, 2, 1], dtype=np.uint32))
        assert e.value.code == BSG_E_INVALID and "ascending" in str(e.value)
    assert int(ctx.device_calls().sum()) == before
