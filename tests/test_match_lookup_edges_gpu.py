"""The lookup walker's probe loops (k_match_rows_lookup*, csrc/match_lookup.hip.h) at the placed edges of tests/lookup_shapes.py: tag
twins, tag extremes, runs that wrap, the full tables with a 60-slot run, role-mixed runs, a collision partner behind the wrap, pair
runs chosen by id arithmetic and the lifetime of the leaf's field id.  Every case goes through bsg_match_rows_lookup and
bsg_match_rows_lookup_rows (the two must expand to the same rows) with one query per condition (TERM c) and the case's composites,
under the default walker, the separator spec and — the families its three-letter namespace builds — the trigram spec, and again
through bsg_match_rows_lookup_regex / _rows with one FieldRegex condition added (the REGEX = true body over the same probes, its blob
behind lanes whose offset depends on the case's table sizes).  Expected bits come from the oracle walker's matcher or the two
tokenizer restatements (lookup_shapes.expected_of), never from the library or the model; the handed-back rows are stated per case:
none, except in collision_behind_the_wrap.  A table of at most 64 conditions must also equal bsg_match_rows_wide byte for byte.
Conditions go in through RawBatch: the collision partner's bytes are not text."""
import numpy as np
import pytest

from bloomsearch_amd import _lib
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from tests import lookup_shapes as LS
from tests.test_match_many_gpu import RawBatch

pytestmark = pytest.mark.gpu

INSTANCES = [(name, walker) for name, case in LS.CASES.items() for walker in case.walkers]


def program(comp):
    """a composite of lookup_shapes as a public postfix program (the nil expression: the empty program)"""
    if comp is None:
        return []
    if isinstance(comp, int):
        return [_lib.op(_lib.OP_TERM, comp)]
    return [o for k in comp[1:] for o in program(k)] + [_lib.op(_lib.OP_AND if comp[0] == "AND" else _lib.OP_OR, len(comp) - 1)]


def kind_of(k):
    return {LS.FIELD: _lib.KIND_FIELD, LS.TOKEN: _lib.KIND_TOKEN, LS.FIELD_TOKEN: _lib.KIND_FIELD_TOKEN, LS.FIELD_REGEX: _lib.KIND_FIELD_REGEX}[k]


def batch_of(case):
    conds = [(kind_of(k), f, t) for k, f, t in case.conds]
    return RawBatch(conds, [program(c) for c in range(len(conds))] + [program(k) for k in case.composites])


def run_case(ctx, case, walker, regex):
    spec = LS.spec_of(walker)
    rows, batch = list(case.rows), batch_of(case)
    nq, n = LS.n_queries(case), len(rows)
    assert len(batch.prog_off) - 1 == nq and n <= 48
    bits_call, rows_call = (ctx.match_rows_lookup_regex, ctx.match_rows_lookup_regex_rows) if regex else (ctx.match_rows_lookup, ctx.match_rows_lookup_rows)
    bits_result = bits_call(rows, batch, tokenizer=spec)
    rows_result = rows_call(rows, batch, tokenizer=spec)
    words, pwo, fb = bits_result
    hdr, poff, payload, fb_rows = rows_result
    assert len(pwo) - 1 == nq == len(hdr) and fb.tobytes() == fb_rows.tobytes()
    assert [int(r) for r in fb] == list(case.handed_back), (case.name, walker)         # stated per case, not computed
    want = LS.expected_of(case, walker)
    decided = np.array([r not in case.handed_back for r in range(n)])
    wrong = []
    for q in range(nq):
        got = wide_pair_bits(words, pwo, q, n)
        listed = pair_rows_list(int(hdr[q]), payload[int(poff[q]): int(poff[q + 1])], n)
        assert np.array_equal(np.flatnonzero(got), listed), (case.name, walker, q)     # both forms expand to the same rows
        assert not got[~decided].any(), (case.name, walker, q)                         # a handed-back row's bits are 0
        if not np.array_equal(got[decided], want[q][decided]):
            wrong.append((q, [int(r) for r in np.flatnonzero(got != (want[q] & decided))]))
    assert not wrong, (case.name, walker, wrong[:8])
    if len(case.conds) <= 64:
        wide = ctx.match_rows_wide(rows, batch, tokenizer=spec)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(wide, bits_result)), (case.name, walker)
        wide_rows = ctx.match_rows_wide_rows(rows, batch, tokenizer=spec)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(wide_rows, rows_result)), (case.name, walker)


@pytest.mark.parametrize("name,walker", INSTANCES, ids=["%s-%s" % i for i in INSTANCES])
def test_lookup(ctx, name, walker):
    run_case(ctx, LS.CASES[name], walker, regex=False)


@pytest.mark.parametrize("name,walker", INSTANCES, ids=["%s-%s" % i for i in INSTANCES])
def test_lookup_regex(ctx, name, walker):
    case = LS.with_regex(LS.CASES[name])
    assert case.conds.count(LS.RX_COND) == 1 and len(case.conds) <= LS.MAX_CONDS
    run_case(ctx, case, walker, regex=True)


def test_the_instances_are_the_ones_the_families_ask_for():
    by_walker = {w: {LS.CASES[n].family for n, x in INSTANCES if x == w} for w in LS.WALKERS}
    assert by_walker["default"] == by_walker["separator"] == set(LS.FAMILIES)
    assert by_walker["trigram"] == set(LS.TRIGRAM_FAMILIES)
    full = [n for n, c in LS.CASES.items() if len(c.conds) == LS.MAX_CONDS]
    assert "long-run" in full and "pair-runs-2048" in full
