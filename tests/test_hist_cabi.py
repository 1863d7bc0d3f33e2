"""bsg_match_rows_wide_hist at the C boundary, without a device: the header declares the call with the parent's first parameters followed
by the eight new ones, the library exports it with those argtypes, BSG_HIST_SLOTS and BSG_HIST_MAX_BUCKETS agree with _lib.py and the
kernel header, a NULL context is refused, the LDS of k_pair_hist is what the header says, and the scanner and the counting pass are
kernels of their own, each launched from one place."""
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
KERNEL = open(os.path.join(CSRC, "hist.hip.h")).read()
NEW_ARGS = ["const uint8_t *field", "uint32_t field_len", "int64_t origin", "uint64_t width", "uint32_t n_buckets", "uint32_t *out_counts",
            "uint32_t *out_fallback_rows", "uint32_t fallback_cap", "uint32_t *out_n_fallback"]


def clean_params(name, text):
    return [re.sub(r"\s*/\*.*?\*/\s*", "", p).strip() for p in params(name, text)]


def test_the_header_declares_the_call_with_the_parents_parameters_then_the_new_ones():
    parent = params("bsg_match_rows_wide_regex_substr_range", GPU_H)
    tok = parent.index("const bsg_tokenizer *tok")
    got = clean_params("bsg_match_rows_wide_hist", GPU_H)
    assert got[: tok + 1] == parent[: tok + 1]
    # field, field_len, origin, width, n_buckets, out_counts, then the parent's fallback list: eight beyond what the parent ends in
    assert got[tok + 1:] == NEW_ARGS and parent[tok + 2:] == NEW_ARGS[6:]
    assert params("bsg_last_hist_ms", GPU_H) == ["bsg_ctx *ctx", "float *hist_ms"]
    block = GPU_H[GPU_H.index("/* ---- Bucketed hit counts"): GPU_H.index("#define BSG_HIST_MAX_BUCKETS")]
    for phrase in ("TOP-LEVEL key", "clamp(floor(v))", "(uint64_t)t - (uint64_t)origin", "q >= n_buckets", "`missing`", "ONE list", "each row once",
                   "counted in no slot", "never scanned, never walked and never handed back", "16 432 bytes", "64 bits", "lookup family"):
        assert phrase in block, phrase


def test_the_library_exports_it_with_the_declared_signature():
    L = _lib.load()
    for name in ("bsg_match_rows_wide_hist", "bsg_last_hist_ms"):
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert len(getattr(L, name).argtypes) == len(params(name, GPU_H)), name
    wide = L.bsg_match_rows_wide_regex_substr_range.argtypes
    got = L.bsg_match_rows_wide_hist.argtypes
    assert got[:16] == wide[:16] and got[16:] == [C.c_void_p, C.c_uint32, C.c_int64, C.c_uint64, C.c_uint32, C.c_void_p] + wide[17:]
    nfb, ms = C.c_uint32(), C.c_float()
    counts = (C.c_uint32 * 8)()
    # without a context the calls refuse, as every entry point does
    assert L.bsg_match_rows_wide_hist(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None,
                                      b"ts", 2, 0, 1, 4, counts, None, 0, C.byref(nfb)) == BSG_E_INVALID
    assert L.bsg_last_hist_ms(None, C.byref(ms)) == BSG_E_INVALID


def define(name, text=GPU_H):
    m = re.search(r"#define %s\s+(\d+)u\b" % name, text)
    assert m, name
    return int(m.group(1))


def test_the_constants_agree_with_the_header_and_the_kernels():
    assert _lib.HIST_MAX_BUCKETS == define("BSG_HIST_MAX_BUCKETS") == constant(KERNEL, "kHistMaxBuckets") == 1024
    assert re.search(r"#define BSG_HIST_SLOTS\(n_buckets\) \(\(n_buckets\) \+ 3u\)", GPU_H)
    assert [_lib.HIST_SLOTS(b) for b in (1, 60, 1024)] == [4, 63, 1027]
    assert constant(KERNEL, "kHistLdsSlots") == _lib.HIST_SLOTS(_lib.HIST_MAX_BUCKETS)
    # four reserved codes no bucket number reaches
    codes = [int(x, 16) for x in re.search(r"kHistBelow = (\w+)u, kHistAbove = (\w+)u, kHistMissing = (\w+)u, kHistUndecided = (\w+)u;", KERNEL).groups()]
    assert len(set(codes)) == 4 and min(codes) >= _lib.HIST_MAX_BUCKETS and max(codes) <= 0xFFFF


def test_the_lds_of_the_counting_pass_is_what_the_header_says():
    assert constant(KERNEL, "kPairHistThreads") == 256
    assert constant(KERNEL, "kPairHistLdsBytes") == 4 * 1027 * 4 == 16432
    assert "static_assert(kPairHistLdsBytes == 16432u" in KERNEL


def test_the_host_call_is_declared_and_exported():
    L = host.lib()
    assert hasattr(L, "bsh_hist_row") and "bsh_hist_row" in host.HOST_EXPORTS
    assert params("bsh_hist_row", HOST_H) == ["const uint8_t *row", "uint64_t len", "const uint8_t *field", "uint32_t field_len", "int64_t origin",
                                              "uint64_t width", "uint32_t n_buckets", "uint32_t *out_slot"]
    assert len(L.bsh_hist_row.argtypes) == 8
    assert L.bsh_hist_row(b"{}", 2, None, 0, 0, 1, 4, None) == -1


def test_the_scanner_and_the_counting_pass_are_kernels_of_their_own():
    for name in ("k_bucket_rows", "k_bucket_rows_sets", "k_pair_hist"):
        assert len(re.findall(r"void %s\(" % name, KERNEL)) == 1, name
    api = open(os.path.join(CSRC, "match_api.inc")).read()
    assert api.count("bsg::k_bucket_rows,") == 1 and api.count("bsg::k_bucket_rows_sets,") == 1 and api.count("bsg::k_pair_hist,") == 1
