"""bsg_match_rows_many_range (k_match_rows_many_range / _tok / _gram): a batch of queries with FieldRange conditions over one table in
one walk.  Plane q is what bsg_match_rows_range returns for program q alone, ANDed with the set mask; rows of a set with mask 0 are
never walked; an exponent literal on the leaf of ANY range condition of the table hands a walked row back."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import substring_restatement as SR

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)


def row(**kv):
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


ROWS = [row(id=i, lat=(i * 7 % 40) / 2, lvl="error" if i % 4 == 0 else "info", **({"x": i % 5} if i % 3 == 0 else {})) for i in range(200)]


def queries(n, gram=False):
    """gram: the tokens of the n-gram walker are 3-rune windows"""
    qs = []
    for q in range(n):
        bloom = [None, Q.FieldToken("lvl", "err" if gram else "error"), Q.Field("x"), Q.Token("inf" if gram else "info")][q % 4]
        rng = [Q.FieldRange("id", q, q + 50), Q.FieldRange("lat", q % 20, None, lo_open=True), Q.RangeOr(Q.FieldRange("x", None, 1), Q.FieldRange("id", 190, None)),
               Q.RangeAnd(Q.FieldRange("lat", None, 10, hi_open=True), Q.FieldRange("id", 3 * q, None)), None][q % 5]
        qs.append((bloom, rng))
    return qs


def singles(ctx, rows, qs, tok):
    out = []
    for bloom, rng in qs:
        hits, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(bloom, rng), tok)
        assert list(fb) == []
        out.append(hits)
    return np.array(out)


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_queries", [1, 2, 63, 64])
def test_plane_q_is_the_single_call_for_program_q(ctx, walker, n_queries):
    tok = SR.WALKERS[walker]
    qs = queries(n_queries, walker == "trigram")
    planes, fb = ctx.match_rows_many_range(ROWS, Q.CompiledRangeQueryBatch(qs), tokenizer=tok)
    assert list(fb) == [] and planes.shape == (n_queries, len(ROWS))
    assert np.array_equal(planes, singles(ctx, ROWS, qs, tok))
    if n_queries <= 2:
        for q, (bloom, rng) in enumerate(qs):
            want = [Hst.match_row_range(rng, r) and (bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) for r in ROWS]
            assert planes[q].tolist() == want and 0 < sum(want) < len(ROWS)


def test_sets_with_masks_and_a_boundary_inside_a_wave(ctx):
    qs = queries(5)
    first = [0, 10, 37, 64, 65, 130, 200]                                       # boundaries at 10 and 37: inside the first wave
    masks = [0b11111, 0, 0b00101, 0b10000, 0, 0b01010]
    planes, fb = ctx.match_rows_many_range(ROWS, Q.CompiledRangeQueryBatch(qs), np.array(first, dtype=np.uint32), np.array(masks, dtype=np.uint64))
    assert list(fb) == []
    alone = singles(ctx, ROWS, qs, None)
    for s, mask in enumerate(masks):
        for q in range(5):
            want = alone[q, first[s]: first[s + 1]] if (mask >> q) & 1 else np.zeros(first[s + 1] - first[s], dtype=bool)
            assert np.array_equal(planes[q, first[s]: first[s + 1]], want), (s, q)
    assert planes.any(axis=1).all()


def test_rows_of_a_set_with_mask_0_are_never_walked(ctx):
    rows = [b'{"v":1e3}', b'{"v":5}', b'{"v":2E1,"w":1}', b'{"v":6}', b'not json', b'{"v":7e0}', b'{"v":7}']
    qs = [(None, Q.FieldRange("v", 5, 7)), (None, Q.FieldRange("w", 1, 1))]
    first, masks = np.array([0, 2, 5, 7], dtype=np.uint32), np.array([0b01, 0, 0b10], dtype=np.uint64)
    planes, fb = ctx.match_rows_many_range(rows, Q.CompiledRangeQueryBatch(qs), first, masks)
    # set 1 (rows 2-4: an exponent literal, a row that is no JSON) is never walked: no fallback rows there.  Row 0 is one for query 0;
    # row 5 is one although its set evaluates only query 1, which does not use the condition on v: ANY condition of the table listens
    assert list(fb) == [0, 5]
    assert planes.tolist() == [[False, True, False, False, False, False, False], [False] * 7]
    assert Hst.match_row_range(qs[0][1], rows[0]) is False and Hst.match_row_range(qs[1][1], rows[5]) is False
    planes, fb = ctx.match_rows_many_range(rows[:4], Q.CompiledRangeQueryBatch(qs))            # no sets: every query on every row
    assert list(fb) == [0, 2] and planes.tolist() == [[False, True, False, True], [False] * 4]


def test_a_table_without_a_range_condition_is_the_parent_call(ctx):
    blooms = [Q.FieldToken("lvl", "error"), Q.Field("x"), None, Q.And(Q.Token("info"), Q.Field("x"))]
    for tok in SR.WALKERS.values():
        a, fa = ctx.match_rows_many_range(ROWS, Q.CompiledMatcherBatch(blooms), tokenizer=tok)
        b, fbk = ctx.match_rows_many(ROWS, Q.CompiledMatcherBatch(blooms), tokenizer=tok)
        assert list(fa) == list(fbk) == [] and np.array_equal(a, b) and a.any()
