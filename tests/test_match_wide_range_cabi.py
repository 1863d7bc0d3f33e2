"""bsg_match_rows_wide_range / bsg_match_rows_wide_range_rows at the C boundary, without a device: the header declares them with the wide
pair's parameter lists, the library exports them with those signatures, both refuse a NULL context, the kind and flag constants of
_lib.py are the header's, the three walkers add no LDS, and the other wide and lookup entry points never set the flag that lets kind 6
pass their kind check."""
import ctypes as C
import os
import re

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID
from tests.test_regex_substr_cabi import constant, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
GPU_H = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()


def test_the_header_declares_both_calls_with_the_wide_pairs_parameters():
    assert params("bsg_match_rows_wide_range", GPU_H) == params("bsg_match_rows_wide", GPU_H)
    assert params("bsg_match_rows_wide_range_rows", GPU_H) == params("bsg_match_rows_wide_rows", GPU_H)
    assert len(params("bsg_match_rows_wide_range", GPU_H)) == 20 and len(params("bsg_match_rows_wide_range_rows", GPU_H)) == 24
    # the contract block states the gate and its difference from the batched call
    block = GPU_H[GPU_H.index("/* bsg_match_rows_wide / bsg_match_rows_wide_rows with range conditions"): GPU_H.index("BSG_API int32_t bsg_match_rows_wide_range(")]
    assert "bsg_match_rows_many_range" in block and "lists a query which uses it" in block and "BSG_E_UNSUPPORTED" in block


def test_the_library_exports_them_with_the_declared_signatures():
    L = _lib.load()
    for name in ("bsg_match_rows_wide_range", "bsg_match_rows_wide_range_rows"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.bsg_match_rows_wide_range.argtypes == L.bsg_match_rows_wide.argtypes
    assert L.bsg_match_rows_wide_range_rows.argtypes == L.bsg_match_rows_wide_rows.argtypes
    assert len(L.bsg_match_rows_wide_range.argtypes) == len(params("bsg_match_rows_wide_range", GPU_H))
    assert len(L.bsg_match_rows_wide_range_rows.argtypes) == len(params("bsg_match_rows_wide_range_rows", GPU_H))
    n, length = C.c_uint32(), C.c_uint64()
    # without a context, and with nothing at all, both refuse like every entry point
    assert L.bsg_match_rows_wide_range(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                       C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_wide_range(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0, None) == BSG_E_INVALID
    assert L.bsg_match_rows_wide_range_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                            C.byref(length), None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_wide_range_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                            None, None, 0, None) == BSG_E_INVALID


def define(name):
    m = re.search(r"#define %s\s+(\d+)u\b" % name, GPU_H)
    assert m, name
    return int(m.group(1))


def test_the_kind_and_flag_constants_agree_with_the_header():
    assert _lib.KIND_FIELD_RANGE == define("BSG_KIND_FIELD_RANGE") == 6
    assert (_lib.KIND_FIELD, _lib.KIND_TOKEN, _lib.KIND_FIELD_TOKEN) == (define("BSG_KIND_FIELD"), define("BSG_KIND_TOKEN"), define("BSG_KIND_FIELD_TOKEN"))
    assert (_lib.KIND_FIELD_REGEX, _lib.KIND_SUBSTRING, _lib.KIND_FIELD_SUBSTRING) == (define("BSG_KIND_FIELD_REGEX"), define("BSG_KIND_SUBSTRING"),
                                                                                      define("BSG_KIND_FIELD_SUBSTRING"))
    assert (_lib.RANGE_NO_LO, _lib.RANGE_NO_HI, _lib.RANGE_LO_OPEN, _lib.RANGE_HI_OPEN) == (define("BSG_RANGE_NO_LO"), define("BSG_RANGE_NO_HI"),
                                                                                          define("BSG_RANGE_LO_OPEN"), define("BSG_RANGE_HI_OPEN"))
    assert len(Q.range_entry({"Field": "v", "Lo": 1})) == define("BSG_RANGE_ENTRY_BYTES") == 17


def test_the_three_walkers_add_no_lds_and_the_body_takes_range_under_wide():
    text = open(os.path.join(CSRC, "ingest.hip.h")).read() + open(os.path.join(CSRC, "match.hip.h")).read()
    wide = constant(text, "kMatchWideLdsBytes")
    assert wide == 35328 and 3 * wide <= 160 * 1024                  # three workgroups per CU, as k_match_rows_store
    assert "static_assert(3u * kMatchWideLdsBytes <= 160u * 1024u" in text
    assert "static_assert(!(RANGE && (REGEX || SUB))," in text and "RANGE && (REGEX || SUB || WIDE)" not in text
    for name in ("k_match_rows_store_range", "k_match_rows_store_range_tok", "k_match_rows_store_range_gram"):
        assert len(re.findall(r"void %s\(" % name, text)) == 1, name
    # the wide mode's range slots hold these kernels and launch with the plain storing walkers' bytes (the range consumer is no substring one)
    api, route = open(os.path.join(CSRC, "match_api.inc")).read(), open(os.path.join(CSRC, "host", "match_route.hpp")).read()
    for suffix, tok in (("", "Default"), ("_tok", "Spec"), ("_gram", "Gram")):
        assert re.search(r"X\(Wide, Range, %s, k_match_rows_store_range%s\)" % (tok, suffix), route), suffix
    assert "case bsh_route::Mode::Wide: return sub ? bsg::kMatchWideSubLdsBytes : bsg::kMatchWideLdsBytes;" in api
    assert "has_substr(Consumers c) { return c == Consumers::Substr || c == Consumers::RegexSubstr || c == Consumers::RegexSubstrRange; }" in route


def test_only_the_two_entry_points_let_kind_6_into_the_wide_call():
    api, route = open(os.path.join(CSRC, "match_api.inc")).read(), open(os.path.join(CSRC, "host", "match_route.hpp")).read()
    accepts = dict(re.findall(r'constexpr CallSpec (k\w+)\{"bsg_match_rows\w*", Mode::\w+, Accepts::(\w+)', route))
    accepts.update({k: accepts[p] for k, p in re.findall(r"constexpr CallSpec (k\w+) = with_policy\((k\w+),", route)})
    assert sorted(k for k, a in accepts.items() if k.startswith(("kWide", "kLookup")) and a == "Range") == ["kWideRange", "kWideRangeRows"]
    for name, spec in (("bsg_match_rows_wide", "kWide"), ("bsg_match_rows_wide_rows", "kWideRows"), ("bsg_match_rows_wide_substr", "kWideSubstr"),
                       ("bsg_match_rows_wide_substr_rows", "kWideSubstrRows"), ("bsg_match_rows_lookup", "kLookup"), ("bsg_match_rows_lookup_rows", "kLookupRows"),
                       ("bsg_match_rows_lookup_regex", "kLookupRegex"), ("bsg_match_rows_lookup_regex_rows", "kLookupRegexRows"),
                       ("bsg_match_rows_wide_range", "kWideRange"), ("bsg_match_rows_wide_range_rows", "kWideRangeRows")):
        entry = api[api.index("int32_t %s(bsg_ctx" % name):]
        assert re.findall(r"bsh_route::(k\w+)", entry[: entry.index("\n}\n")]) == [spec], name
        assert accepts[spec] in (("Range",) if "range" in name else ("Plain", "Regex", "RegexSubstr")), name      # kind 6 passes only the two
    body = api[api.index("int32_t match_rows_wide_call("): api.index("}  // namespace", api.index("int32_t match_rows_wide_call("))]
    # kinds 3-5 are named and unsupported, a kind above 6 unknown, and the bounds are built by the function the other range calls use
    assert "if (int32_t rc = route_call(mc, n_queries)) return rc;" in body
    assert "if (acc == Accepts::Range && k >= kKindFieldRegex && k <= kKindFieldSubstring) return refuse(Refusal::TextWithRange, c, k);" in route
    assert re.search(r'case Refusal::TextWithRange:\s+return fail\(BSG_E_UNSUPPORTED, "condition %u: kind %u \(the range calls hold', api)
    assert 'case Refusal::UnknownKind: return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, kind);' in api
    assert "acc == Accepts::Range ? kKindFieldRange : kKindFieldSubstring;" in route
    assert api.count("build_range_table(mc)") == 1 and api.count("int32_t build_range_table(") == 1


def test_the_wide_batch_holds_any_number_of_range_queries():
    pairs = [(Q.FieldToken("lvl", "err") if q % 2 else None, Q.FieldRange("ts", 100 * (q % 7), None) if q % 3 else Q.RangeOr(Q.FieldRange("ts", None, q % 5),
                                                                                                                         Q.FieldRange("st", 500, None)))
             for q in range(200)]
    b = Q.CompiledWideRangeBatch(pairs)
    assert isinstance(b, Q.CompiledRangeQueryBatch) and b.n_queries == 200 and len(b.kinds) == 1 + 7 + 5 + 1
    one = Q.CompiledRangeQueryBatch(pairs[:64])
    assert b.prog_ops[: b.prog_off[64]] == one.prog_ops and b.kinds[: len(one.kinds)] == one.kinds
