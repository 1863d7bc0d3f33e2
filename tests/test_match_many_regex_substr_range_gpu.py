"""bsg_match_rows_many_regex_substr_range (k_match_rows_many_regex_substr_range / _tok / _gram): a batch of queries over one table that
holds FieldRange conditions beside FieldRegex and substring ones.  Plane q is compared with the restatements
(tests/range_text_cases.want) under the set mask, and with the single call bsg_match_rows_regex_substr_range on query q."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests.range_text_cases import row, want
from tests.test_match_regex_substr_gpu import AT_MANY_CAP, OVER_MANY_CAP, counted
from tests.test_match_regex_substr_range_gpu import cap_rows, unsupported

pytestmark = pytest.mark.gpu

WALKERS = RT.WALKERS
MSGS = ["connection timeout", "Connection reset by peer", "cache miss: timeout", "all good", "retry 3 of 5", "peer closed connection"]
REGEXES = [Q.FieldRegex("msg", "timeout|cache"), Q.FieldRegex("lvl", "^err"), Q.FieldRegex("msg", "timeout|retry"), Q.FieldRegex("ts", "^17")]
SUBS = [Q.Substring("reset by"), Q.FieldSubstring("peer", "10.0.3."), Q.Substring("0000"), Q.FieldSubstring("msg", "CONN")]
RANGES = [Q.FieldRange("ts", 1700000000, 1700000050), Q.FieldRange("ts", 1700000100, None, lo_open=True), Q.FieldRange("lat", None, 50, hi_open=True),
          Q.FieldRange("lat", 60, 80)]
# every (regex, substring, range) triple of the pools, each side also missing in some: 64 queries over ONE table of 12 conditions
QUERIES = [(Q.FieldToken("lvl", "err") if q % 5 == 0 else None, REGEXES[q % 4] if q % 7 else None, SUBS[(q // 4) % 4] if q % 11 else None, RANGES[q // 16])
           for q in range(64)]
ROWS = 140
FIRST = np.array([0, 40, 100, 140], dtype=np.uint32)          # both inner boundaries lie inside a wave


def make_rows():
    rng = np.random.default_rng(23)
    return [row(msg=MSGS[rng.integers(0, len(MSGS))], lvl=["err", "inf"][rng.integers(0, 2)], peer="10.%d.3.%d" % (rng.integers(0, 2), i), ts=1700000000 + i,
                lat=int(rng.integers(0, 200)) / 2) for i in range(ROWS)]


@pytest.fixture(scope="module")
def rows():
    return make_rows()


@pytest.fixture(scope="module")
def expected(rows):
    """want() of every query under every walker, computed once"""
    return {w: [want(rows, *q, SR.WALKERS[w]) for q in QUERIES] for w in WALKERS}


def test_the_batch_shares_one_table():
    b = Q.CompiledRowTextRangeQueryBatch(QUERIES)
    assert b.n_queries == 64 and len(b.kinds) == 13
    assert b.kinds.count(_lib.KIND_FIELD_REGEX) == 4 and b.kinds.count(_lib.KIND_FIELD_RANGE) == 4 and b.kinds.count(_lib.KIND_FIELD_TOKEN) == 1


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_queries", [1, 2, 64])
def test_plane_q_is_the_single_call_for_program_q(ctx, rows, expected, walker, n_queries):
    tok = SR.WALKERS[walker]
    base = 4 if n_queries < 64 else 0
    queries = QUERIES[base: base + n_queries]
    batch = Q.CompiledRowTextRangeQueryBatch(queries)
    planes, fb = ctx.match_rows_many_regex_substr_range(rows, batch, tokenizer=tok)
    assert list(fb) == [] and planes.shape == (n_queries, ROWS)
    for q, quad in enumerate(queries):
        w = expected[walker][base + q]
        assert np.array_equal(planes[q], w), q
        single, sfb = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowTextRangeQuery(*quad), tok)
        assert list(sfb) == [] and np.array_equal(single, planes[q]), q
    assert any(p.any() for p in planes) and not all(p.all() for p in planes)


@pytest.mark.parametrize("walker", WALKERS)
def test_set_masks_with_a_boundary_inside_a_wave(ctx, rows, expected, walker):
    tok = SR.WALKERS[walker]
    idx = [7, 21, 36, 42]                                       # a low window of ts, a high one, two of lat
    queries = [QUERIES[i] for i in idx]
    masks = np.array([0b0111, 0, 0b1010], dtype=np.uint64)
    batch = Q.CompiledRowTextRangeQueryBatch(queries)
    planes, fb = ctx.match_rows_many_regex_substr_range(rows, batch, FIRST, masks, tok)
    assert list(fb) == []
    sizes = np.diff(FIRST)
    for q in range(4):
        on = np.repeat([(int(m) >> q) & 1 == 1 for m in masks], sizes)
        assert np.array_equal(planes[q], expected[walker][idx[q]] & on), q
    assert not planes[:, 40:100].any() and planes[:, :40].any() and planes[:, 100:].any()
    # rows no walker can decide, in the set with mask 0: not walked, so bit 0 and not handed back
    bad = list(rows)
    bad[43] = b'{"msg":"connection re'
    bad[64] = ('{"msg":"connection %s reset"}' % RT.unassigned_rune()).encode()
    bad[99] = b'{"ts":17e8,"msg":"timeout"}'
    again, fb = ctx.match_rows_many_regex_substr_range(bad, batch, FIRST, masks, tok)
    assert list(fb) == [] and np.array_equal(again, planes)
    again, fb = ctx.match_rows_many_regex_substr_range(bad, batch, FIRST, np.array([0b0111, 0b0100, 0b1010], dtype=np.uint64), tok)
    assert list(fb) == [43, 64, 99] and not again[:, [43, 64, 99]].any()


@pytest.mark.parametrize("walker", WALKERS)
def test_a_regex_condition_of_a_masked_out_query_does_not_count(ctx, walker):
    """query 0 puts four regex conditions on the leaf `a`, query 1 a fifth: a row of a set that evaluates both is handed back, a row
    of a set on which query 1 is masked off is decided (a lane holds four)"""
    tok = SR.WALKERS[walker]
    queries = [(None, Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^err", "a", ".")]), Q.Substring("needle"), Q.FieldRange("n", 1, 9)),
               (None, Q.FieldRegex("a", "timeout|cache"), Q.Substring("x n"), Q.FieldRange("n", 5, None)),
               (None, None, Q.FieldSubstring("a", "NEEDLE"), Q.FieldRange("n", None, 5))]
    batch = Q.CompiledRowTextRangeQueryBatch(queries)
    rows = [b'{"a":"err: x and a needle","n":3}', b'{"b":"x needle","n":5}', b'{"a":"cache x needle","n":7}'] * 2
    first = np.array([0, 3, 6], dtype=np.uint32)
    planes, fb = ctx.match_rows_many_regex_substr_range(rows, batch, first, np.array([0b101, 0b111], dtype=np.uint64), tok)
    assert list(fb) == [3, 5]                                   # only where the row's set evaluates all five
    w = [want(rows, *q, tok) for q in queries]
    assert w[0].tolist() == [True, False, False] * 2 and w[1].tolist() == [False, False, True] * 2 and w[2].tolist() == [True, False, False] * 2
    decided = np.array([True, True, True, False, True, False])
    assert np.array_equal(planes[0], w[0] & decided)
    assert np.array_equal(planes[1], w[1] & decided & np.array([False] * 3 + [True] * 3))
    assert np.array_equal(planes[2], w[2] & decided)


@pytest.mark.parametrize("walker", WALKERS)
def test_an_exponent_literal_hands_its_row_back_whatever_the_mask(ctx, walker):
    """ANY range condition of the table listens: the row goes back although the only query that reads the condition is masked off on
    its set; under mask 0 the row is not walked at all"""
    tok = SR.WALKERS[walker]
    queries = [(None, Q.FieldRegex("m", "timeout"), None, Q.FieldRange("v", 1000, 1000)), (None, None, Q.Substring("timeout"), Q.FieldRange("u", 1, 1))]
    batch = Q.CompiledRowTextRangeQueryBatch(queries)
    rows = [b'{"v":1e3,"u":1,"m":"timeout"}', b'{"v":1000,"u":1,"m":"timeout"}', b'{"w":1e3,"v":1000,"u":2,"m":"timeout"}'] * 3
    first = np.array([0, 3, 6, 9], dtype=np.uint32)
    planes, fb = ctx.match_rows_many_regex_substr_range(rows, batch, first, np.array([0b11, 0b10, 0], dtype=np.uint64), tok)
    assert list(fb) == [0, 3]
    assert planes[0].tolist() == [False, True, True] + [False] * 6
    assert planes[1].tolist() == [False, True, False, False, True, False] + [False] * 3
    w = [want(rows, *q, tok) for q in queries]
    assert w[0].tolist() == [True, True, True] * 3 and w[1].tolist() == [True, True, False] * 3


@pytest.mark.parametrize("walker", WALKERS)
def test_the_largest_blob_beside_a_range_condition(ctx, walker):
    """34 032 bytes of regex tables, user masks included, with or without a needle in the table; four bytes more are refused before
    any launch"""
    tok = SR.WALKERS[walker]
    rows, rg = cap_rows(AT_MANY_CAP), Q.FieldRange("n", 5, 5)
    at, over = Q.RegexOr(*counted(AT_MANY_CAP)), Q.RegexOr(*counted(OVER_MANY_CAP))
    for sx, bits in ((Q.FieldSubstring("z", "needle"), [1, 0, 0, 0, 0]), (None, [1, 0, 1, 0, 0])):
        queries = [(None, at, sx, rg), (None, counted(AT_MANY_CAP)[-1], None, None), (None, None, sx, rg)]
        planes, fb = ctx.match_rows_many_regex_substr_range(rows, Q.CompiledRowTextRangeQueryBatch(queries), tokenizer=tok)
        assert list(fb) == []
        assert planes[0].tolist() == [bool(b) for b in bits] and planes[1].tolist() == [True, False, False, False, False]
        assert planes[2].tolist() == ([True, True, False, False, True] if sx else [True, True, True, False, True])
        for q, quad in enumerate(queries):
            assert np.array_equal(planes[q], want(rows, *quad, tok)), q
        before = int(ctx.device_calls().sum())
        assert "LDS" in unsupported(ctx.match_rows_many_regex_substr_range, rows, Q.CompiledRowTextRangeQueryBatch([(None, over, sx, rg)]), None, None, tok)
        assert int(ctx.device_calls().sum()) == before
    # without a range condition the table is bsg_match_rows_many_regex's, under its own cap
    planes, fb = ctx.match_rows_many_regex_substr_range(rows, Q.CompiledRowTextRangeQueryBatch([(None, over, None, None)]), tokenizer=tok)
    assert list(fb) == [] and planes[0].tolist() == [False, False, True, True, False]
