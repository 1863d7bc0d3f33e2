"""The MinMax calls at the C boundary, without a device: the header declares bsg_ingest_rows_minmax / bsg_ingest_open_minmax with the
parent calls' parameters plus the three field arguments, the library exports them with those signatures, every new call refuses a
NULL context, the constants of _lib.py and the kernel header are the header's, bsg_minmax and bsg_ingest_stats have their stated
sizes, and the scanner is a kernel of its own beside the walkers."""
import ctypes as C
import os
import re

from bloomsearch_amd import _lib, host
from bloomsearch_amd._lib import BSG_E_INVALID
from tests.test_regex_substr_cabi import constant, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
GPU_H = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
HOST_H = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()
FIELD_ARGS = ["const uint8_t *field_bytes", "const uint32_t *field_off", "uint32_t n_fields"]


def test_the_header_declares_the_calls_with_the_parents_parameters_plus_three():
    assert params("bsg_ingest_rows_minmax", GPU_H) == params("bsg_ingest_rows_tok", GPU_H) + FIELD_ARGS
    assert params("bsg_ingest_open_minmax", GPU_H) == params("bsg_ingest_open", GPU_H) + FIELD_ARGS
    assert params("bsg_ingest_minmax", GPU_H) == ["bsg_ctx *ctx", "uint64_t ingest_id", "bsg_minmax *out", "uint64_t cap"]
    assert params("bsg_last_minmax_ms", GPU_H) == ["bsg_ctx *ctx", "float *minmax_ms"]
    # the streaming calls keep their signatures
    assert len(params("bsg_ingest_append_rows", GPU_H)) == 9 and len(params("bsg_ingest_add_sets", GPU_H)) == 6
    block = GPU_H[GPU_H.index("/* ---- per-set MinMax indexes"): GPU_H.index("#define BSG_MINMAX_MAX_FIELDS")]
    for phrase in ("TOP-LEVEL key", "LAST counts", "clamp(floor(v))", "literal with an exponent", "contains a backslash", "HAS\n * inserted its bloom entries",
                   "bit-identical"):
        assert phrase in block, phrase


def test_the_library_exports_them_with_the_declared_signatures():
    L = _lib.load()
    for name in ("bsg_ingest_rows_minmax", "bsg_ingest_open_minmax", "bsg_ingest_minmax", "bsg_last_minmax_ms"):
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert len(getattr(L, name).argtypes) == len(params(name, GPU_H)), name
    assert L.bsg_ingest_rows_minmax.argtypes[:-3] == L.bsg_ingest_rows_tok.argtypes
    assert L.bsg_ingest_open_minmax.argtypes[:-3] == L.bsg_ingest_open.argtypes
    out, ms = C.c_uint64(), C.c_float()
    names, off = (C.c_uint8 * 2)(116, 115), (C.c_uint32 * 2)(0, 2)
    # without a context every call refuses, as every entry point does
    assert L.bsg_ingest_rows_minmax(None, None, None, 0, None, 0, None, 0, None, 0, None, C.byref(out), names, off, 1) == BSG_E_INVALID
    assert L.bsg_ingest_open_minmax(None, 0, None, 0, None, 0, None, C.byref(out), names, off, 1) == BSG_E_INVALID
    assert L.bsg_ingest_minmax(None, 1, None, 0) == BSG_E_INVALID
    assert L.bsg_last_minmax_ms(None, C.byref(ms)) == BSG_E_INVALID


def define(name, text=GPU_H):
    m = re.search(r"#define %s\s+(\d+)u\b" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_constants_and_the_record_agree_with_the_header():
    assert _lib.MINMAX_MAX_FIELDS == define("BSG_MINMAX_MAX_FIELDS") == 8
    assert _lib.MINMAX_MAX_NAME == define("BSG_MINMAX_MAX_NAME") == 64
    kernel = open(os.path.join(CSRC, "minmax.hip.h")).read()
    assert constant(kernel, "kMinMaxMaxFields") == 8 and constant(kernel, "kMinMaxMaxName") == 64
    assert re.search(r"typedef struct bsg_minmax \{\s*int64_t min, max;[^}]*uint32_t present;[^}]*uint32_t reserved;\s*\} bsg_minmax;", GPU_H)
    assert _lib.MINMAX_DTYPE.itemsize == 24 and _lib.MINMAX_DTYPE.names == ("min", "max", "present", "reserved")
    assert "static_assert(sizeof(MinMaxRec) == 24" in kernel
    # bsg_ingest_stats keeps its layout: the scanner's time has a call of its own
    assert C.sizeof(_lib.IngestStats) == 48
    stats = GPU_H[GPU_H.index("typedef struct bsg_ingest_stats {"): GPU_H.index("} bsg_ingest_stats;")]
    assert "minmax" not in stats and re.findall(r"(?:uint32_t|uint64_t|float) (\w+);", stats) == [
        "n_rows", "n_fallback_rows", "table_grows", "reserved", "row_bytes", "table_bytes", "ms_walk", "ms_union", "ms_build", "ms_encode"]
    ops = [define("BSH_MM_" + n, HOST_H) for n in ("EQ", "NE", "GT", "GE", "LT", "LE", "IN", "NOT_IN", "BETWEEN", "NOT_BETWEEN")]
    assert ops == list(range(10)) == [host.MM_OPS[n] for n in ("EQ", "NE", "GT", "GTE", "LT", "LTE", "IN", "NOT_IN", "BETWEEN", "NOT_BETWEEN")]


def test_the_host_calls_are_declared_and_exported():
    L = host.lib()
    for name in ("bsh_minmax_row", "bsh_minmax_eval", "bsh_prefilter_eval"):
        assert hasattr(L, name) and name in host.HOST_EXPORTS
        assert len(getattr(L, name).argtypes) == len(params(name, HOST_H)), name
    assert L.bsh_minmax_row(b"{}", 2, None, None, 1, None) == -1 and L.bsh_minmax_eval(None, 0, 0, None, 0, 0, 0) == -1


def test_the_scanner_is_a_kernel_of_its_own():
    kernel = open(os.path.join(CSRC, "minmax.hip.h")).read()
    for name in ("k_minmax_rows", "k_minmax_rows_sets"):
        assert len(re.findall(r"void %s\(" % name, kernel)) == 1, name
    walkers = open(os.path.join(CSRC, "ingest.hip.h")).read()
    assert "minmax" not in walkers.lower()                         # no seventh consumer inside ingest_rows_body
    api = open(os.path.join(CSRC, "ingest_api.inc")).read()
    chunk_loop = api[api.index("int32_t walk_chunks("): api.index("// ---- MinMax indexes (minmax.hip.h)")]
    # once per chunk, on the first attempt only: never again when the walk is re-run after a table grew
    assert chunk_loop.count("once(c, rf, re)") == 1
    first = chunk_loop[chunk_loop.index("if (!first_attempt)"): chunk_loop.index("bsg::IngestArgs b = a;")]
    assert first.index("else {") < first.index("once(c, rf, re)")
    assert api.count("bsg::k_minmax_rows,") == 1 and api.count("bsg::k_minmax_rows_sets,") == 1
