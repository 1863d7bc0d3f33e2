"""bsg_match_rows_many_regex_substr (k_match_rows_many_regex_substr / _tok / _gram): a batch of queries over one table that holds
FieldRegex AND substring conditions.  Plane q is compared with the restatements (tests/test_match_regex_substr_gpu.want: bloom,
Python `re`, substring restatement) under the set mask, and with the single call bsg_match_rows_regex_substr on query q."""
import json

import numpy as np
import pytest

from bloomsearch_amd import query as Q
from bloomsearch_amd._lib import KIND_FIELD_REGEX, KIND_FIELD_SUBSTRING, KIND_SUBSTRING
from tests import substring_restatement as SR
from tests.test_match_regex_substr_gpu import want

pytestmark = pytest.mark.gpu

N_SETS, SET_ROWS = 3, 70
MSGS = ["connection timeout", "Connection reset by peer", "cache miss: timeout", "all good", "retry 3 of 5", "peer closed connection"]
# a regex-only query, a substring-only query, one with both sides, and one with all three
QUERIES = [
    (None, Q.RegexOr(Q.FieldRegex("msg", "timeout|cache"), Q.FieldRegex("lvl", "^err")), None),
    (None, None, Q.SubstringOr(Q.Substring("reset by"), Q.FieldSubstring("peer", "10.0.3."))),
    (None, Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3.")),
    (Q.FieldToken("lvl", "err"), Q.FieldRegex("msg", "timeout|cache"), Q.FieldSubstring("msg", "CONN")),
]


def make_rows():
    rng = np.random.default_rng(17)
    rows = []
    for i in range(N_SETS * SET_ROWS):
        d = {"msg": MSGS[rng.integers(0, len(MSGS))], "lvl": ["err", "inf"][rng.integers(0, 2)], "peer": "10.%d.3.%d" % (rng.integers(0, 2), i)}
        rows.append(json.dumps(d, separators=(",", ":")).encode())
    return rows


@pytest.fixture(scope="module")
def rows():
    return make_rows()


def test_the_batch_shares_one_table_of_eight_conditions():
    b = Q.CompiledRowSubstringQueryBatch(QUERIES)
    assert b.n_queries == 4 and len(b.kinds) == 8
    assert b.kinds.count(KIND_FIELD_REGEX) == 3 and b.kinds.count(KIND_SUBSTRING) == 2 and b.kinds.count(KIND_FIELD_SUBSTRING) == 2


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_plane_q_is_query_q_under_the_set_mask(ctx, rows, walker):
    tok = SR.WALKERS[walker]
    first = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
    masks = np.array([0b1111, 0b0101, 0b1010], dtype=np.uint64)
    batch = Q.CompiledRowSubstringQueryBatch(QUERIES)
    planes, fb = ctx.match_rows_many_regex_substr(rows, batch, first, masks, tok)
    assert list(fb) == [] and planes.shape == (4, len(rows))
    every, fb = ctx.match_rows_many_regex_substr(rows, batch, tokenizer=tok)         # without a set table: every query on every row
    assert list(fb) == []
    for q, (bloom, rx, sx) in enumerate(QUERIES):
        w = want(rows, bloom, rx, sx, tok)
        on = np.repeat([(int(m) >> q) & 1 == 1 for m in masks], SET_ROWS)
        assert np.array_equal(planes[q], w & on), q
        assert np.array_equal(every[q], w), q
        assert w[on].any() and not w.all()
        single, sfb = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, rx, sx), tok)
        assert list(sfb) == [] and np.array_equal(single, w)


def test_a_set_with_mask_0_is_never_walked(ctx, rows):
    """the middle set holds rows no walker can decide (cut-off JSON, a rune the lower table does not know): under mask 0 they are
    not walked, so they are no fallback rows and their plane bits are 0; under a non-zero mask they are handed back"""
    bad = list(rows)
    bad[SET_ROWS + 3] = b'{"msg":"connection re'
    bad[SET_ROWS + 9] = '{"msg":"connection \u0378 reset"}'.encode()
    first = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
    batch = Q.CompiledRowSubstringQueryBatch(QUERIES)
    planes, fb = ctx.match_rows_many_regex_substr(bad, batch, first, np.array([0b1111, 0, 0b1111], dtype=np.uint64))
    assert list(fb) == [] and not planes[:, SET_ROWS: 2 * SET_ROWS].any()
    good, _ = ctx.match_rows_many_regex_substr(rows, batch, first, np.array([0b1111, 0, 0b1111], dtype=np.uint64))
    assert np.array_equal(planes, good) and planes.any()
    planes, fb = ctx.match_rows_many_regex_substr(bad, batch, first, np.array([0b1111, 0b0001, 0b1111], dtype=np.uint64))
    assert list(fb) == [SET_ROWS + 3, SET_ROWS + 9] and not planes[:, [SET_ROWS + 3, SET_ROWS + 9]].any()


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_five_regex_conditions_on_one_leaf_count_only_those_of_the_rows_queries(ctx, walker):
    """query 0 puts four regex conditions on the leaf `a`, query 1 a fifth: a row of a set that evaluates both is handed back, a row
    of a set on which query 1 is masked off is decided (a lane holds four)"""
    tok = SR.WALKERS[walker]
    queries = [(None, Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^err", "a", ".")]), Q.Substring("needle")),
               (None, Q.FieldRegex("a", "timeout|cache"), Q.Substring("x n")),
               (None, None, Q.FieldSubstring("a", "NEEDLE"))]
    batch = Q.CompiledRowSubstringQueryBatch(queries)
    rows = [b'{"a":"err: x and a needle"}', b'{"b":"x needle"}', b'{"a":"cache x needle"}'] * 2
    first = np.array([0, 3, 6], dtype=np.uint32)
    planes, fb = ctx.match_rows_many_regex_substr(rows, batch, first, np.array([0b101, 0b111], dtype=np.uint64), tok)
    assert list(fb) == [3, 5]                                   # only where the row's set evaluates all five
    w = [want(rows, *q, tok) for q in queries]
    assert w[0].tolist() == [True, False, False] * 2 and w[1].tolist() == [False, False, True] * 2 and w[2].tolist() == [True, False, True] * 2
    decided = np.array([True, True, True, False, True, False])
    assert np.array_equal(planes[0], w[0] & decided)
    assert np.array_equal(planes[1], w[1] & decided & np.array([False] * 3 + [True] * 3))
    assert np.array_equal(planes[2], w[2] & decided)
