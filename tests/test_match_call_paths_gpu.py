"""What the row-matcher families share (csrc/match_api.inc: one call record, one prologue, one part runner, one walker launcher, one
fan-out): bsg_match_rows_regex per query, bsg_match_rows_many_regex, and bsg_match_rows_wide with the implicit set and with an
explicit set table answer the same five queries over the same rows with the same bits and the same fallback list — on one device
with the default chunk (the reference), with 64 KiB chunks, cut over two and three devices, and under a separator-family tokenizer."""
import numpy as np
import pytest

from bloomsearch_amd import query as Q, synth
from bloomsearch_amd.gpu import Context, wide_pair_bits
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_match_many_gpu import BAD_ROWS

pytestmark = pytest.mark.gpu

N_ROWS = 1500
BAD_AT = [0, 63, 64, N_ROWS - 1]
SET_FIRST = [0, 700, 700, N_ROWS]                                                      # three sets, the middle one empty; 700 is no multiple of 64
RX = Q.FieldRegex("service", "^(auth|pay)")
# one table: Field, Token, FieldToken and one FieldRegex condition; five (bloom, regex) queries over it
QUERIES = [(Q.FieldToken("level", "error"), None), (Q.Token("timeout"), RX), (Q.Field("nested.az"), None),
           (Q.Or(Q.Token("error"), Q.FieldToken("service", "auth")), RX), (None, RX)]


class Case:
    def __init__(self):
        self.rows = synth.rows_json(7000, N_ROWS)
        for i, r in enumerate(BAD_AT):
            self.rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
        assert sum(len(r) for r in self.rows) >= 3 * (1 << 16)                         # at least three chunks of the smallest size
        self.singles = [Q.CompiledRowQuery(*q) for q in QUERIES]
        self.many = Q.CompiledRowQueryBatch(QUERIES)
        self.wide = Q.CompiledWideBatch(QUERIES)
        assert sorted(set(self.wide.kinds)) == [0, 1, 2, 3] and list(self.wide.kinds).count(3) == 1
        nq = len(QUERIES)
        self.set_off = [0, nq, 2 * nq, 3 * nq]                                         # every query on every set, the empty one included
        self.set_queries = list(range(nq)) * 3

    def families(self, ctx, tokenizer=None, n_dev=None):
        """-> {family: (bool [n_queries, n_rows], fallback rows)}; n_dev: every call must have used exactly that many devices"""
        rows, nq = self.rows, len(QUERIES)
        out = {}

        def counted(fn):
            before = ctx.device_calls()
            res = fn()
            if n_dev is not None:
                assert int(((ctx.device_calls() - before) > 0).sum()) == n_dev
            return res

        one = [counted(lambda m=m: ctx.match_rows_regex(rows, m, tokenizer=tokenizer)) for m in self.singles]
        out["single"] = (np.array([h for h, _ in one], dtype=bool), sorted(set(int(r) for _, fb in one for r in fb)))
        planes, fb = counted(lambda: ctx.match_rows_many_regex(rows, self.many, tokenizer=tokenizer))
        out["many"] = (np.asarray(planes, dtype=bool), [int(r) for r in fb])
        words, pwo, fb = counted(lambda: ctx.match_rows_wide(rows, self.wide, tokenizer=tokenizer))
        out["wide"] = (np.array([wide_pair_bits(words, pwo, q, N_ROWS) for q in range(nq)]), [int(r) for r in fb])
        words, pwo, fb = counted(lambda: ctx.match_rows_wide(rows, self.wide, SET_FIRST, self.set_off, self.set_queries, tokenizer=tokenizer))
        assert len(pwo) == 3 * nq + 1 and int(pwo[2 * nq]) == int(pwo[nq])            # the empty set's pairs own no word
        sets = [np.array([wide_pair_bits(words, pwo, s * nq + q, SET_FIRST[s + 1] - SET_FIRST[s]) for q in range(nq)]).reshape(nq, -1) for s in range(3)]
        out["wide sets"] = (np.concatenate(sets, axis=1), [int(r) for r in fb])
        return out

    def check(self, got, want):
        for name, (bits, fb) in got.items():
            assert bits.shape == (len(QUERIES), N_ROWS), name
            assert np.array_equal(bits, want[0]), name
            assert fb == want[1], name


@pytest.fixture(scope="module")
def case(ctx):
    c = Case()
    ref = c.families(ctx, n_dev=1)
    c.reference = ref["single"]
    c.all_reference = ref
    return c


def test_the_families_agree_on_one_device(case):
    bits, fb = case.reference
    assert fb == BAD_AT and not bits[:, BAD_AT].any()
    assert all(int(bits[q].sum()) > 0 for q in range(len(QUERIES))) and not bits[1].all()
    d = synth.draws(7000, N_ROWS)
    good = np.ones(N_ROWS, dtype=bool)
    good[BAD_AT] = False
    assert np.array_equal(bits[0], (d["level"] == synth.LEVELS.index("error")) & good)  # the generator's ground truth for query 0
    case.check(case.all_reference, case.reference)


def test_the_families_agree_in_64_kib_chunks(ctx, case):
    try:
        ctx.set_ingest_chunk(1 << 16)
        got = case.families(ctx, n_dev=1)
    finally:
        ctx.set_ingest_chunk(0)
    case.check(got, case.reference)


@pytest.mark.parametrize("n_dev", [2, 3])
def test_the_families_agree_cut_over_devices(case, n_dev):
    with Context(device_ids(n_dev)) as m:
        m.set_lab(7, 1)                                                                # every call is cut over the devices, however small
        m.set_lab(8, 1)
        got = case.families(m, n_dev=n_dev)
    case.check(got, case.reference)


def test_the_families_agree_under_a_separator_tokenizer(ctx, case):
    got = case.families(ctx, tokenizer=TR.SPECS["punct_lower"], n_dev=1)
    assert got["single"][1] == BAD_AT and got["single"][0].sum() > 0
    case.check(got, got["single"])
