"""One call per walker slot of the row matcher's route table (csrc/host/match_route.hpp): 4 modes x the consumer sets x 3 tokenizers =
60 kernels.  For each slot an entry point, a table and a tokenizer that the route (restated in tests/test_match_route.py) sends
there; the bits, and the rows the walker hands back decided by the host, are compared exactly with bloomsearch_amd/host.py's matchers.
2 x kIngestThreads + 1 rows (193 when a workgroup holds 128): more than one workgroup, more than one 64-lane word, a ragged last word.
Every side of a query has a row that matches and one that does not, and two rows are outside the walker's envelope.  The batched and
wide slots get two sets with different queries, the lookup slots a table with a repeated condition.  The test does not try to observe
which kernel ran: a kernel in another slot's place shows as a wrong bit or a launch that fails."""
import os
import re

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd._lib import OP_TERM, op
from bloomsearch_amd.gpu import wide_pair_bits
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests import test_match_route as RS
from tests import walker_envelope_shapes as WE
from tests.range_text_cases import row
from tests.test_match_regex_substr_range_gpu import host_verdict
from tests.test_match_wide_range_gpu import csr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INGEST_THREADS = int(re.search(r"constexpr int kIngestThreads = (\d+);", open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "ingest.hip.h")).read()).group(1))
N_ROWS = 193 if INGEST_THREADS == 128 else 2 * INGEST_THREADS + 1
CUT = N_ROWS // 2 + 3                            # the second set begins inside a word
HANDED_BACK = [70, CUT + 30]                     # one row per set outside the walker's envelope
TOKENIZERS = {"Default": SR.WALKERS["default"], "Spec": SR.WALKERS["separators"], "Gram": SR.WALKERS["trigram"]}

# the sides of the two queries: each slot's queries take the bloom side and the sides of its consumer set
BLOOM = (Q.Token("err"), Q.And(Q.Token("inf"), Q.Field("peer")))
REGEX = (Q.FieldRegex("msg", "timeout|retry"), Q.FieldRegex("peer", "^10\\.1"))
SUBSTR = (Q.Substring("10.0.3."), Q.FieldSubstring("msg", "cache"))
RANGE = (Q.FieldRange("ts", 1700000040, 1700000000 + CUT + 60), Q.FieldRange("lat", None, 40))
SIDES = {"None": (0, 0, 0), "Regex": (1, 0, 0), "Substr": (0, 1, 0), "RegexSubstr": (1, 1, 0), "Range": (0, 0, 1), "RegexSubstrRange": (1, 1, 1)}
SINGLE = {"None": "match_rows", "Regex": "match_rows_regex", "Substr": "match_rows_substr", "RegexSubstr": "match_rows_regex_substr", "Range": "match_rows_range",
          "RegexSubstrRange": "match_rows_regex_substr_range"}
MANY = {c: m.replace("match_rows", "match_rows_many") for c, m in SINGLE.items()}
WIDE = {"None": "match_rows_wide", "Regex": "match_rows_wide", "Substr": "match_rows_wide_substr", "RegexSubstr": "match_rows_wide_substr",
        "Range": "match_rows_wide_range", "RegexSubstrRange": "match_rows_wide_regex_substr_range"}
LOOKUP = {"None": "match_rows_lookup", "Regex": "match_rows_lookup_regex"}
SLOTS = [(m, c, t) for m in RS.MODES for c in RS.SETS for t in RS.TOKS if m != "Lookup" or c in LOOKUP]


def make_rows():
    rows = [row(msg=("upstream timeout", "cache warm", "retry later")[i % 3], lvl=("err", "inf")[(i // 2) % 2], peer="10.%d.3.%d" % (i % 5 == 0, i),
                ts=1700000000 + i, lat=(i * 7) % 90) for i in range(N_ROWS)]
    rows[HANDED_BACK[0]] = RT.DEEP17
    rows[HANDED_BACK[1]] = b'{"lvl":"err","msg":"upstream time'
    assert not any(WE.in_envelope(rows[i]) for i in HANDED_BACK[:1])
    return rows


ROWS = make_rows()
_verdicts = {}


def verdicts(quad, tok_name):
    """the four host matchers over every row, asked once per (query, tokenizer)"""
    key = (repr(quad), tok_name)
    if key not in _verdicts:
        _verdicts[key] = np.array([host_verdict(r, *quad, TOKENIZERS[tok_name]) for r in ROWS], dtype=bool)
    return _verdicts[key]


def queries_of(cset):
    rx, sx, rg = SIDES[cset]
    return [(BLOOM[q], REGEX[q] if rx else None, SUBSTR[q] if sx else None, RANGE[q] if rg else None) for q in range(2)]


class Table:
    """a batch's table and programs as given (the lookup slots: with a condition repeated behind the table and a query on the copy)"""

    def __init__(self, batch, repeat=None):
        self.kinds, self.fields, self.tokens = list(batch.kinds), list(batch.fields), list(batch.tokens)
        self.prog_ops, self.prog_off = list(batch.prog_ops), list(batch.prog_off)
        if repeat is not None:
            self.kinds.append(self.kinds[repeat]); self.fields.append(self.fields[repeat]); self.tokens.append(self.tokens[repeat])
            self.prog_ops.append(op(OP_TERM, len(self.kinds) - 1))
            self.prog_off.append(len(self.prog_ops))


def check_routed(mode, cset, kinds, name):
    """the restated route sends this entry point's table to the slot under test"""
    e = RS.expected(name, list(kinds), 2)
    assert isinstance(e, dict) and RS.SPECS[name][0] == mode and e["set"] == cset, (name, e)


def decided(got, fb, want):
    """device bits outside the handed-back rows, the host's verdict on those: the call's answer is the host's on every row"""
    assert not got[fb].any()
    final = got.copy()
    final[fb] = want[fb]
    assert np.array_equal(final, want)


@pytest.mark.parametrize("mode,cset,tok_name", SLOTS, ids=["-".join(s) for s in SLOTS])
def test_every_slot_answers_as_the_host_matchers(ctx, mode, cset, tok_name):
    tok = TOKENIZERS[tok_name]
    queries = queries_of(cset)
    want = [verdicts(q, tok_name) for q in queries]
    for q, quad in enumerate(queries):             # a matching and a non-matching row per side and per query
        assert 0 < want[q].sum() < N_ROWS
        for side in range(4):
            if quad[side] is not None:
                alone = verdicts(tuple(quad[s] if s == side else None for s in range(4)), tok_name)
                assert 0 < alone.sum() < N_ROWS, (q, side)
    first = np.array([0, CUT, N_ROWS], dtype=np.uint32)
    in_set = [np.arange(N_ROWS) < CUT, np.arange(N_ROWS) >= CUT]
    if mode == "Single":
        m = Q.CompiledRowTextRangeQuery(*queries[0])
        check_routed(mode, cset, m.kinds, "bsg_" + SINGLE[cset] if tok is None or cset not in ("None", "Regex") else "bsg_match_rows_tok")
        got, fb = getattr(ctx, SINGLE[cset])(ROWS, m, tok)
        assert list(fb) == HANDED_BACK
        decided(got, fb, want[0])
    elif mode == "Many":                           # set 0 asks both queries, set 1 the second
        batch = Q.CompiledRowTextRangeQueryBatch(queries)
        check_routed(mode, cset, batch.kinds, "bsg_" + MANY[cset])
        planes, fb = getattr(ctx, MANY[cset])(ROWS, batch, first, np.array([0b11, 0b10], dtype=np.uint64), tok)
        assert list(fb) == HANDED_BACK
        decided(planes[0], fb, want[0] & in_set[0])
        decided(planes[1], fb, want[1])
    else:                                          # set 0 lists both queries, set 1 the second (the lookup slots: and the query on the copy)
        batch = Q.CompiledWideTextRangeBatch(queries)
        table = Table(batch, repeat=0 if mode == "Lookup" else None)
        method = (LOOKUP if mode == "Lookup" else WIDE)[cset]
        check_routed(mode, cset, table.kinds, "bsg_" + method)
        lists = [[0, 1], [1, 2]] if mode == "Lookup" else [[0, 1], [1]]
        if mode == "Lookup":
            assert table.kinds[0] == table.kinds[-1] and table.tokens[0] == table.tokens[-1] == b"err"
            queries.append((Q.Token("err"), None, None, None))
            want.append(verdicts(queries[2], tok_name))
        off, sq = csr(lists)
        words, pwo, fb = getattr(ctx, method)(ROWS, table, first, off, sq, tok)
        assert list(fb) == HANDED_BACK
        p = 0
        for s, listed in enumerate(lists):
            lo, hi = int(first[s]), int(first[s + 1])
            here = np.array([r - lo for r in fb if lo <= r < hi], dtype=np.int64)
            for q in listed:
                decided(wide_pair_bits(words, pwo, p, hi - lo), here, want[q][lo:hi])
                p += 1
