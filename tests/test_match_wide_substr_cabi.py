"""bsg_match_rows_wide_substr / bsg_match_rows_wide_substr_rows at the C boundary, without a device: the header declares them with the
wide pair's parameter lists, the library exports them, the three LDS constants of the instances satisfy the sums their
static_asserts state, and the wide call itself still refuses the kinds."""
import ctypes as C
import os
import re

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID
from tests.test_regex_substr_cabi import constant, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")


def test_the_header_declares_both_calls_with_the_wide_pairs_parameters():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert params("bsg_match_rows_wide_substr", gpu_h) == params("bsg_match_rows_wide", gpu_h)
    assert params("bsg_match_rows_wide_substr_rows", gpu_h) == params("bsg_match_rows_wide_rows", gpu_h)
    assert len(params("bsg_match_rows_wide_substr", gpu_h)) == 20 and len(params("bsg_match_rows_wide_substr_rows", gpu_h)) == 24
    # the contract block states both caps as numbers
    block = gpu_h[gpu_h.index("/* bsg_match_rows_wide / bsg_match_rows_wide_rows with substring conditions"): gpu_h.index("BSG_API int32_t bsg_match_rows_wide_substr(")]
    assert "42 496" in block and "46 592" in block and "39 424" in block


def test_the_library_exports_them():
    L = _lib.load()
    for name in ("bsg_match_rows_wide_substr", "bsg_match_rows_wide_substr_rows"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.bsg_match_rows_wide_substr.argtypes == L.bsg_match_rows_wide.argtypes
    assert L.bsg_match_rows_wide_substr_rows.argtypes == L.bsg_match_rows_wide_rows.argtypes
    n, length = C.c_uint32(), C.c_uint64()
    # without a context both refuse like every entry point
    assert L.bsg_match_rows_wide_substr(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                        C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_wide_substr_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                             C.byref(length), None, 0, C.byref(n)) == BSG_E_INVALID


def test_the_lds_constants_satisfy_the_stated_sums():
    text = open(os.path.join(CSRC, "ingest.hip.h")).read() + open(os.path.join(CSRC, "match.hip.h")).read()
    wide, wide_sub, cap = constant(text, "kMatchWideLdsBytes"), constant(text, "kMatchWideSubLdsBytes"), constant(text, "kRxWideSubLdsCap")
    assert wide == 35328 and wide % 16 == 0                  # the needle table behind the lanes: M[b] stays one aligned 16-byte read
    assert wide_sub == 35328 + 4096 == 39424 and 3 * wide_sub <= 163840          # three workgroups per CU
    assert cap == 81920 - 39424 == 42496 and cap <= 0x10000 and 2 * (wide_sub + cap) <= 163840      # 16-bit blob offsets; two workgroups per CU
    assert cap < constant(text, "kRxWideLdsCap") == 46592
    groups = open(os.path.join(CSRC, "host", "regex_groups.hpp")).read()
    assert constant(groups, "kWideSubLdsCap") == cap
    assert "static_assert(!(SUB && WIDE)" not in text


def test_the_wide_call_still_refuses_the_kinds():
    api, route = open(os.path.join(CSRC, "match_api.inc")).read(), open(os.path.join(CSRC, "host", "match_route.hpp")).read()
    body = api[api.index("int32_t match_rows_wide_call("): api.index("}  // namespace", api.index("int32_t match_rows_wide_call("))]
    # kinds 4 and 5 pass the kind check only under the specs the two new entry points name (and the calls that take every kind)
    assert "if (int32_t rc = route_call(mc, n_queries)) return rc;" in body
    assert 'case Refusal::UnknownKind: return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, kind);' in api
    assert "if (k > max_kind) return refuse(Refusal::UnknownKind, c, k);" in route
    accepts = dict(re.findall(r'constexpr CallSpec (k\w+)\{"bsg_match_rows\w*", Mode::\w+, Accepts::(\w+)', route))
    accepts.update({k: accepts[p] for k, p in re.findall(r"constexpr CallSpec (k\w+) = with_policy\((k\w+),", route)})
    assert sorted(k for k, a in accepts.items() if k.startswith("kWide") and a == "RegexSubstr") == ["kWideSubstr", "kWideSubstrRows"]
    assert all(accepts[k] in ("Plain", "Regex") for k in ("kWide", "kWideRows", "kLookup", "kLookupRows", "kLookupRegex", "kLookupRegexRows"))
    for name, spec in (("bsg_match_rows_wide", "kWide"), ("bsg_match_rows_wide_rows", "kWideRows"), ("bsg_match_rows_lookup", "kLookup"),
                       ("bsg_match_rows_lookup_rows", "kLookupRows"), ("bsg_match_rows_lookup_regex", "kLookupRegex"),
                       ("bsg_match_rows_lookup_regex_rows", "kLookupRegexRows"), ("bsg_match_rows_wide_substr", "kWideSubstr"),
                       ("bsg_match_rows_wide_substr_rows", "kWideSubstrRows")):
        entry = api[api.index("int32_t %s(bsg_ctx" % name):]
        assert re.findall(r"bsh_route::(k\w+)", entry[: entry.index("\n}\n")]) == [spec], name


def test_the_wide_batch_holds_any_number_of_substring_queries():
    triples = [(Q.FieldToken("lvl", "err") if q % 2 else None, Q.FieldRegex("msg", "a|b") if q % 3 == 0 else None, Q.Substring("n%d" % (q % 5))) for q in range(200)]
    b = Q.CompiledWideSubstringBatch(triples)
    assert isinstance(b, Q.CompiledRowSubstringQueryBatch) and b.n_queries == 200 and len(b.kinds) == 7
    one = Q.CompiledRowSubstringQueryBatch(triples[:64])
    assert b.prog_ops[: b.prog_off[64]] == one.prog_ops and b.kinds[: len(one.kinds)] == one.kinds
