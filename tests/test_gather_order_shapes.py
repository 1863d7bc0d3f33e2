"""tests/gather_order_shapes.py (the gather kernels' order of a lane's locations and their phase walk, restated) against the oracle's
per-term membership on small filters, and against tools/probe_gather_lab.py's `lines` rows on a 64-block sample of the bench's arena
and batch.  No GPU.

The sample's index-order figures against the 1 000-block figures on record (204.8 tests, 144.5 lines per block, {1,3,6}).  A block's
test count is 17 present terms x 10 plus, for each of the 12 absent terms, 1 / 4 / 10 tests with probability 1/2, 7/16, 1/16 (it dies
in the phase that meets its first clear bit, bits set with probability 1/2): variance 5.5 per term, 66 per block, so the mean of 64
blocks has a standard deviation of 1.0 test; four of them: 4.1.  Lines: L (1 - exp(-t / L)) at L = 275 moves by 0.47 per test (0.5
for the tests' deviation), and the occupancy of 275 lines by ~205 tests has itself a standard deviation below 5 per block (0.6 for
the mean); together 0.8, four of them: 3.2."""
import importlib.util
import os

import numpy as np
import pytest

from bloomsearch_amd import query as Q, synth
from bloomsearch_amd.arena import plan_blocks
from oracle import oracle as O
from tests import gather_order_shapes as S
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lab():
    spec = importlib.util.spec_from_file_location("probe_gather_lab", os.path.join(ROOT, "tools", "probe_gather_lab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sample():
    """64 blocks of the bench's arena and the bench's batch -> words, desc, term strings, kinds, and the restatement's walk per order"""
    from benchlib import common as bench
    plan = plan_blocks(bench.generate_blocks(np.arange(64, dtype=np.int64), 10000, 0xB100F5EA4C4, 1), 0.001)
    words = H.oracle_words(plan)
    cb = Q.compile_queries(synth.make_queries(4096, "c2", seed=1234))
    kinds = [int(v) for v in cb.arrays()[2]]
    walks = {o: S.walk_arena(words, plan.desc, cb.term_strings, kinds, o) for o in ("index", "line")}
    return words, plan.desc, cb.term_strings, kinds, walks


def small_arena(fpr, rows=200, n_blocks=9, absent=frozenset()):
    plan = plan_blocks([synth.block_entry_sets(b * rows, rows) for b in range(n_blocks)], fpr, absent=set(absent))
    return H.oracle_words(plan), plan.desc


TERMS = [Q.FieldToken("level", v) for v in synth.LEVELS + ["absent-level-1"]] + [Q.FieldToken("service", v) for v in synth.SERVICES[:3] + ["absent-svc-2"]] + \
        [Q.FieldToken("nested.region", "region-%d" % r) for r in (0, 3, 7, 9)] + [Q.Token("error"), Q.Token("absent-token"), Q.Field("nested.az"), Q.Field("no.such.field")]


@pytest.mark.parametrize("fpr,k", [(0.7, 1), (0.3, 2), (0.08, 4), (0.001, 10), (0.00002, 16), (0.00001, 17), (1e-6, 20)])
def test_verdicts_are_the_oracles_membership_in_either_order(fpr, k):
    words, desc = small_arena(fpr, absent=frozenset({(3, 2)}))
    assert int(desc["k"][2]) == k and int(desc["m"][3 * 3 + 2]) == 0
    cb = Q.compile_queries(TERMS)
    ops, poff, kinds = cb.arrays()
    want = O.probe_batch(words, desc.view(O.DESC_DTYPE), H.oracle_terms(cb).view(O.TERM_DTYPE), ops, poff)      # one query per term
    n_blocks = len(desc) // 3
    for order in ("index", "line"):
        got = S.walk_arena(words, desc, cb.term_strings, [int(v) for v in kinds], order)
        for b in range(n_blocks):
            tests, lines, per_phase, verdicts = got[b]
            assert verdicts == [bool((int(want[q, 0]) >> b) & 1) for q in range(len(TERMS))], (order, b)
            assert lines <= per_phase <= tests
    assert not all(got[0][3]) and any(got[0][3])


def test_the_line_order_is_a_permutation_sorted_by_line_then_index():
    h = O.base_hashes(b"level::error")
    for m, k in ((1024, 10), (1025, 10), (35000, 10), (35000, 16), (35000, 17), (1 << 27, 10), ((1 << 27) + 1, 10), ((1 << 31) + 5, 10)):
        locs = S.locations(h, m, k)
        seq = S.ordered(locs, m, "line")
        assert sorted(seq) == list(range(k))
        if k <= 16 and m <= 1 << 27:
            assert all((locs[a] >> 10, a) < (locs[b] >> 10, b) for a, b in zip(seq, seq[1:]))
        else:
            assert seq == list(range(k))
    assert S.ordered(S.locations(h, 1024, 10), 1024, "line") == list(range(10))                # one line: every key equal, the index decides
    assert S.phases(10) == [(0, 1), (1, 3), (4, 6)] and S.phases(2) == [(0, 1), (1, 1)] and S.phases(17) == [(0, 1), (1, 3), (4, 6), (10, 6), (16, 1)]


def test_a_word_with_two_equal_locations_is_found():
    s, i, j = S.a_word_with_two_equal_locations(1025, 10)
    locs = S.locations(O.base_hashes(s.encode()), 1025, 10)
    assert i < j and locs[i] == locs[j] and s == s.lower()


def test_the_restatement_equals_the_lab_tool_rows(lab, sample):
    words, desc, strings, kinds, walks = sample
    h = np.asarray([O.base_hashes(s if isinstance(s, bytes) else s.encode()) for s in strings], dtype=np.uint64)
    res, _, verdict = lab.touched_lines(words, desc, h, np.asarray(kinds, dtype=np.int64), (S.SCHEDULE, (4, 4, 2)), ("index", "line"))
    B = len(desc) // 3
    for order in ("index", "line"):
        for sch in (S.SCHEDULE, (4, 4, 2)):
            w = walks[order] if sch == S.SCHEDULE else S.walk_arena(words, desc, strings, kinds, order, sch)
            tests, lines, per_phase = res[(order, sch)]
            assert (round(tests * B), round(lines * B), round(per_phase * B)) == (sum(x[0] for x in w), sum(x[1] for x in w), sum(x[2] for x in w)), (order, sch)
    assert [list(v) for v in verdict] == [x[3] for x in walks["line"]] == [x[3] for x in walks["index"]]


def test_index_order_reproduces_the_figures_on_record(sample):
    w = sample[4]["index"]
    tests, lines = sum(x[0] for x in w) / 64, sum(x[1] for x in w) / 64
    print("index order, 64 blocks: %.2f tests, %.2f lines per block" % (tests, lines))
    assert abs(tests - 204.8) <= 4.1 and abs(lines - 144.5) <= 3.2


def test_line_order_asks_for_fewer_lines_phase_by_phase(sample):
    """what the order is for: the same tests within the sampling error, fewer distinct lines summed phase by phase"""
    wi, wl = sample[4]["index"], sample[4]["line"]
    print("per-phase sums: index %.2f, line %.2f" % (sum(x[2] for x in wi) / 64, sum(x[2] for x in wl) / 64))
    assert sum(x[2] for x in wl) < sum(x[2] for x in wi)
    assert any(a[0] != b[0] for a, b in zip(wi, wl))          # the orders execute different tests: the GPU test can tell them apart
