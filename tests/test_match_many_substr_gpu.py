"""bsg_match_rows_many_substr (k_match_rows_many_substr / _tok / _gram): a batch of queries over one table with Substring and
FieldSubstring conditions.  Plane q is compared with the single call bsg_match_rows_substr for program q (itself checked against
the host matcher in test_match_substr_gpu.py) ANDed with the set mask, and with the host matcher directly."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd._lib import KIND_FIELD_SUBSTRING, KIND_SUBSTRING
from tests import substring_restatement as SR

pytestmark = pytest.mark.gpu

N_SETS, SET_ROWS = 3, 70
MSGS = ["connection timeout", "Connection reset by peer", "Timeout waiting for lock", "all good", "disk full: /var", "peer closed connection"]
# 5 queries over 6 distinct conditions: Token(all), FieldToken(lvl, err), Field(x), Substring(timeout), Substring(l go), FieldSubstring(msg, conn);
# the tokens have at most 3 runes, so they are tokens under the trigram spec too
QUERIES = [
    (Q.Token("all"), Q.Substring("l go")),
    (None, Q.SubstringOr(Q.Substring("timeout"), Q.FieldSubstring("msg", "conn"))),
    (Q.FieldToken("lvl", "err"), Q.FieldSubstring("msg", "conn")),
    (Q.Or(Q.Field("x"), Q.Token("all")), Q.SubstringAnd(Q.Substring("timeout"), Q.FieldSubstring("msg", "conn"))),
    (Q.FieldToken("lvl", "err"), None),
]


def make_rows():
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


def test_the_batch_shares_six_conditions():
    b = Q.CompiledSubstringQueryBatch(QUERIES)
    assert b.n_queries == 5 and len(b.kinds) == 6 and b.kinds.count(KIND_SUBSTRING) == 2 and b.kinds.count(KIND_FIELD_SUBSTRING) == 1


@pytest.mark.parametrize("walker", sorted(SR.WALKERS))
def test_plane_q_is_the_single_call_for_program_q_under_the_set_mask(ctx, rows, walker):
    tok = SR.WALKERS[walker]
    first = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
    masks = np.array([0b11111, 0b01010, 0b10101], dtype=np.uint64)
    planes, fb = ctx.match_rows_many_substr(rows, Q.CompiledSubstringQueryBatch(QUERIES), first, masks, tok)
    assert list(fb) == [] and planes.shape == (5, len(rows))
    for q, (bloom, sub) in enumerate(QUERIES):
        single, sfb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(bloom, sub), tok)
        assert list(sfb) == []
        host = np.array([Hst.match_row_substring(sub, r, tok) and (bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) for r in rows])
        assert np.array_equal(single, host)
        on = np.repeat([(int(m) >> q) & 1 == 1 for m in masks], SET_ROWS)
        assert np.array_equal(planes[q], single & on), q
        assert single[on].any() and not single.all()
    # without a set table: every query on every row
    every, fb = ctx.match_rows_many_substr(rows, Q.CompiledSubstringQueryBatch(QUERIES), tokenizer=tok)
    assert list(fb) == []
    for q, (bloom, sub) in enumerate(QUERIES):
        assert np.array_equal(every[q], ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(bloom, sub), tok)[0])


def test_a_set_with_mask_0_is_never_walked(ctx, rows):
    """the middle set holds rows no walker can decide (cut-off JSON, a rune the lower table does not know): under mask 0 they are
    not walked, so they are no fallback rows and their plane bits are 0; under a non-zero mask they are handed back"""
    bad = list(rows)
    bad[SET_ROWS + 3] = b'{"msg":"connection re'
    bad[SET_ROWS + 9] = '{"msg":"connection \u0378 reset"}'.encode()
    first = np.arange(N_SETS + 1, dtype=np.uint32) * SET_ROWS
    batch = Q.CompiledSubstringQueryBatch(QUERIES)
    planes, fb = ctx.match_rows_many_substr(bad, batch, first, np.array([0b11111, 0, 0b11111], dtype=np.uint64))
    assert list(fb) == [] and not planes[:, SET_ROWS: 2 * SET_ROWS].any()
    good, _ = ctx.match_rows_many_substr(rows, batch, first, np.array([0b11111, 0, 0b11111], dtype=np.uint64))
    assert np.array_equal(planes, good)
    planes, fb = ctx.match_rows_many_substr(bad, batch, first, np.array([0b11111, 0b00001, 0b11111], dtype=np.uint64))
    assert list(fb) == [SET_ROWS + 3, SET_ROWS + 9] and not planes[:, [SET_ROWS + 3, SET_ROWS + 9]].any()
