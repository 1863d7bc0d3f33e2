"""bsg_match_rows_wide_regex_substr_range / bsg_match_rows_wide_regex_substr_range_rows at the C boundary, without a GPU: the header
declares them with the wide calls' parameter lists, the built library exports them, query.CompiledWideTextRangeBatch lowers more than
64 (bloom, regex, substring, range) quadruples into one table, the three storing walkers exist and launch with the regex_substr
instances' LDS, and the literal bits of tests/range_text_cases.EDGES are still what the restatements say."""
import ctypes as C
import os
import re

import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests.test_match_many_regex_substr_range_gpu import RANGES, REGEXES, SUBS
from tests.test_regex_substr_cabi import constant, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
NEW = ("bsg_match_rows_wide_regex_substr_range", "bsg_match_rows_wide_regex_substr_range_rows")
# every (regex, substring, range) triple of the batched suite's pools, each side also missing in some: 70 queries over ONE table
QUERIES = [(Q.FieldToken("lvl", "err") if q % 5 == 0 else None, REGEXES[q % 4] if q % 7 else None, SUBS[(q // 4) % 4] if q % 11 else None, RANGES[(q // 16) % 4])
           for q in range(70)]


def test_the_header_declares_both_calls_with_the_wide_calls_parameters():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert params(NEW[0], gpu_h) == params("bsg_match_rows_wide", gpu_h) and len(params(NEW[0], gpu_h)) == 20
    assert params(NEW[1], gpu_h) == params("bsg_match_rows_wide_rows", gpu_h) and len(params(NEW[1], gpu_h)) == 24


def test_the_library_exports_them():
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS
    n, length = C.c_uint32(), C.c_uint64()
    # without a context both refuse like every entry point
    assert L.bsg_match_rows_wide_regex_substr_range(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                                    C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_wide_regex_substr_range_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None,
                                                         None, 0, C.byref(length), None, 0, C.byref(n)) == BSG_E_INVALID


def test_seventy_queries_share_one_table_of_at_most_sixteen_conditions():
    b = Q.CompiledWideTextRangeBatch(QUERIES)
    assert b.n_queries == 70 > 64 and len(b.kinds) == 13 <= 16
    assert b.kinds.count(_lib.KIND_FIELD_REGEX) == 4 and b.kinds.count(_lib.KIND_FIELD_RANGE) == 4 and b.kinds.count(_lib.KIND_FIELD_TOKEN) == 1
    assert b.kinds.count(_lib.KIND_SUBSTRING) == 2 and b.kinds.count(_lib.KIND_FIELD_SUBSTRING) == 2
    assert len(b.prog_off) == 71
    with pytest.raises(ValueError):
        Q.CompiledRowTextRangeQueryBatch(QUERIES)                    # the batched call's batch holds 64
    # the first 64 programs and the table are the batched class's own
    small = Q.CompiledRowTextRangeQueryBatch(QUERIES[:64])
    assert (small.kinds, small.fields, small.tokens) == (b.kinds, b.fields, b.tokens)
    assert list(b.prog_ops[: small.prog_off[-1]]) == list(small.prog_ops) and list(b.prog_off[:65]) == list(small.prog_off)


@pytest.mark.parametrize("walker", RT.WALKERS)
def test_the_literal_bits_of_the_edge_cases_are_still_the_restatements(walker):
    RT.check_edges_against_the_restatements(SR.WALKERS[walker])


def test_the_three_storing_walkers_launch_with_the_regex_substr_instances_lds():
    text = open(os.path.join(CSRC, "ingest.hip.h")).read() + open(os.path.join(CSRC, "match.hip.h")).read()
    wide_sub = constant(text, "kMatchWideSubLdsBytes")
    assert constant(text, "kRxWideSubLdsCap") == 42496 == 80 * 1024 - wide_sub and wide_sub == constant(text, "kMatchWideLdsBytes") + 4096
    assert 2 * (wide_sub + 42496) <= 160 * 1024 < 3 * (wide_sub + 42496) and 3 * wide_sub <= 160 * 1024      # two workgroups per CU with a blob at the cap, three without one
    body = open(os.path.join(CSRC, "match.hip.h")).read()
    for suffix in ("", "_tok", "_gram"):
        assert re.search(r"void k_match_rows_store_regex_substr_range%s\(const MatchArgs a, const RxArgs x, const SubArgs sb, const MatchWideArgs wd" % suffix, body), suffix
    assert "range conditions beside the text consumers: the single and the batched walkers only" not in body
    # the wide mode's three-consumer slots hold these kernels, every slot with the substring consumer launches with the needle table's
    # bytes, and the three-consumer route builds its blob under the cap beside that table
    api, route = open(os.path.join(CSRC, "match_api.inc")).read(), open(os.path.join(CSRC, "host", "match_route.hpp")).read()
    for suffix, tok in (("", "Default"), ("_tok", "Spec"), ("_gram", "Gram")):
        assert re.search(r"X\(Wide, RegexSubstrRange, %s, k_match_rows_store_regex_substr_range%s\)" % (tok, suffix), route), suffix
    assert "case bsh_route::Mode::Wide: return sub ? bsg::kMatchWideSubLdsBytes : bsg::kMatchWideLdsBytes;" in api
    assert re.search(r"has_substr\(Consumers c\) \{ return [^}]*c == Consumers::RegexSubstrRange; \}", route)
    assert "case bsh_route::Cap::WideSub: return bsh_rxg::kWideSubLdsCap;" in api and "case Mode::Wide: return beside_needles ? Cap::WideSub : Cap::Wide;" in route
    assert re.search(r"case Accepts::All:[^\n]*\n\s+r\.blob = r\.needles = r\.range_table = true; r\.cap = cap_of\(s\.mode, true\);", route)
