"""The range calls at the C boundary: a plain C99 program links bsg_match_rows_range / bsg_match_rows_many_range and bsh_match_row_range;
the headers declare them with the argument lists of bsg_match_rows_tok / bsg_match_rows_many; and (on a GPU: every check of these
calls sits behind the context) what they refuse before anything is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst
from bloomsearch_amd._lib import BSG_E_INVALID, BSG_E_UNSUPPORTED
from bloomsearch_amd.gpu import pack_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "bloomgpu.h"
#include "bloomsearch_host.h"

int main(void)
{
    static const char rows[] = "{\"ts\":1700000005,\"l\":\"a\"}{\"ts\":1700000050.5}";
    const uint64_t row_off[3] = {0, 25, 44};
    /* ts in [1700000000, 1700000010]; ts > 1700000050 (no upper bound) */
    uint8_t conds[2 + BSG_RANGE_ENTRY_BYTES + 2 + BSG_RANGE_ENTRY_BYTES];
    static const char tree[] = "{\"ExpressionType\":\"CONDITION\",\"Condition\":{\"Field\":\"ts\",\"Lo\":1700000050,\"LoOpen\":true}}";
    const uint32_t cond_off[5] = {0, 2, 2 + BSG_RANGE_ENTRY_BYTES, 4 + BSG_RANGE_ENTRY_BYTES, 4 + 2 * BSG_RANGE_ENTRY_BYTES};
    const uint32_t kinds[2] = {BSG_KIND_FIELD_RANGE, BSG_KIND_FIELD_RANGE};
    const uint32_t prog[1] = {BSG_OP(BSG_OP_TERM, 0)}, progs[2] = {BSG_OP(BSG_OP_TERM, 0), BSG_OP(BSG_OP_TERM, 1)}, prog_off[3] = {0, 1, 2};
    const int64_t lo0 = 1700000000, hi0 = 1700000010, lo1 = 1700000050;
    uint64_t bits[2] = {0, 0};
    uint32_t fb[2], nfb = 7;
    bsg_ctx *ctx = NULL;
    int ids[1] = {0};
    int32_t rc;
    int i;
    memset(conds, 0, sizeof conds);
    memcpy(conds, "ts", 2);
    memcpy(conds + 2 + BSG_RANGE_ENTRY_BYTES, "ts", 2);
    for (i = 0; i < 8; ++i) {                                /* little-endian whatever the host */
        conds[2 + i] = (uint8_t)((uint64_t)lo0 >> (8 * i));
        conds[10 + i] = (uint8_t)((uint64_t)hi0 >> (8 * i));
        conds[4 + BSG_RANGE_ENTRY_BYTES + i] = (uint8_t)((uint64_t)lo1 >> (8 * i));
    }
    conds[18] = 0;
    conds[4 + BSG_RANGE_ENTRY_BYTES + 16] = BSG_RANGE_NO_HI | BSG_RANGE_LO_OPEN;
    /* without a context both calls refuse like every entry point */
    if (bsg_match_rows_range(NULL, (const uint8_t *)rows, row_off, 2, conds, cond_off, kinds, 2, prog, 1, NULL, bits, fb, 2, &nfb) != BSG_E_INVALID) return 1;
    if (bsg_match_rows_many_range(NULL, (const uint8_t *)rows, row_off, 2, conds, cond_off, kinds, 2, progs, prog_off, 2, NULL, NULL, 0, NULL, bits, fb, 2,
                                  &nfb) != BSG_E_INVALID) return 2;
    /* the host side needs no device */
    if (bsh_match_row_range(tree, strlen(tree), (const uint8_t *)rows + 25, 19) != 1) return 3;
    if (bsh_match_row_range(tree, strlen(tree), (const uint8_t *)rows, 25) != 0) return 4;
    if (bsh_match_row_range("{", 1, (const uint8_t *)rows, 25) >= 0) return 5;
    rc = bsg_open(ids, 1, &ctx);
    printf("open=%d\n", rc);
    if (rc == BSG_OK) {
        if (bsg_match_rows_range(ctx, (const uint8_t *)rows, row_off, 2, conds, cond_off, kinds, 2, prog, 1, NULL, bits, fb, 2, &nfb) != BSG_OK) return 6;
        if (nfb != 0 || bits[0] != 1) return 7;
        if (bsg_match_rows_many_range(ctx, (const uint8_t *)rows, row_off, 2, conds, cond_off, kinds, 2, progs, prog_off, 2, NULL, NULL, 0, NULL, bits, fb, 2,
                                      &nfb) != BSG_OK) return 8;
        if (nfb != 0 || bits[0] != 1 || bits[1] != 2) return 9;
        printf("matched\n");
        bsg_close(ctx);
    } else if (rc != BSG_E_NODEVICE) {
        return 10;
    }
    return 0;
}
"""


def run_c_caller(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "no gcc"
    src = tmp_path / "range_caller.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "range_caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libbloomgpu.so", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    return out.stdout


def test_a_plain_c99_program_links_the_range_calls(tmp_path):
    out = run_c_caller(tmp_path)
    if _lib.load().bsg_device_count() == 0:
        assert "open=-6" in out


@pytest.mark.gpu
def test_the_c_program_matches_on_the_device(tmp_path):
    assert "matched" in run_c_caller(tmp_path)


def test_the_headers_declare_the_calls_with_their_parents_arguments():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    host_h = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()

    def params(name, text):
        m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, text)
        assert m, name
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params("bsg_match_rows_range", gpu_h) == params("bsg_match_rows_tok", gpu_h)
    assert params("bsg_match_rows_many_range", gpu_h) == params("bsg_match_rows_many", gpu_h) and len(params("bsg_match_rows_many", gpu_h)) == 19
    assert "#define BSG_KIND_FIELD_RANGE      6u" in gpu_h and "#define BSG_RANGE_ENTRY_BYTES 17u" in gpu_h
    assert len(params("bsh_match_row_range", host_h)) == 4 and len(params("bsh_prune_query_range", host_h)) == len(params("bsh_prune_query_sub", host_h)) + 2
    L = _lib.load()
    Hst.lib()
    for name in ("bsg_match_rows_range", "bsg_match_rows_many_range", "bsh_match_row_range", "bsh_prune_query_range"):
        assert hasattr(L, name) and name in _lib.EXPORTS + Hst.HOST_EXPORTS
    assert _lib.KIND_FIELD_RANGE == 6 and (_lib.RANGE_NO_LO, _lib.RANGE_NO_HI, _lib.RANGE_LO_OPEN, _lib.RANGE_HI_OPEN) == (1, 2, 4, 8)
    n = C.c_uint32()
    assert L.bsg_match_rows_range(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_many_range(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID


# ---- what the calls refuse before a launch ----
ROWS = [b'{"v":5,"m":"abc"}', b'{"v":7}']
ENTRY = (5).to_bytes(8, "little", signed=True) + (6).to_bytes(8, "little", signed=True)


def call(ctx, kinds, fields, tokens, fn="bsg_match_rows_range"):
    """-> the status of one raw call over ROWS (single: the program TERM 0; batched: that one query), the bits, the fallback count"""
    L = ctx.L
    off = np.array([0, len(ROWS[0]), len(ROWS[0]) + len(ROWS[1])], dtype=np.uint64)
    blob = np.frombuffer(b"".join(ROWS), dtype=np.uint8)
    cblob, coff = pack_entries([s for pair in zip(fields, tokens) for s in pair])
    kinds = np.asarray(kinds, dtype=np.uint32)
    ops = np.asarray([_lib.op(_lib.OP_TERM, 0)], dtype=np.uint32)
    poff = np.array([0, len(ops)], dtype=np.uint32)
    bits, fb, nfb = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint32), C.c_uint32()
    head = (ctx.h, _lib._ptr(blob), _lib._ptr(off), 2, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds), len(kinds), _lib._ptr(ops))
    tail = (_lib._ptr(bits), _lib._ptr(fb), 2, C.byref(nfb))
    if fn in ("bsg_match_rows", "bsg_match_rows_regex"):
        return getattr(L, fn)(*head, len(ops), *tail), int(bits[0]), nfb.value
    if "many" not in fn and "wide" not in fn and "lookup" not in fn:
        return getattr(L, fn)(*head, len(ops), None, *tail), int(bits[0]), nfb.value
    if "many" in fn:
        return getattr(L, fn)(*head, poff.ctypes.data, 1, None, None, 0, None, *tail), int(bits[0]), nfb.value
    return getattr(L, fn)(*head, poff.ctypes.data, 1, None, None, None, 0, None, *tail), int(bits[0]), nfb.value


def last_error(ctx):
    return ctx.L.bsg_last_error(ctx.h).decode()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["bsg_match_rows_range", "bsg_match_rows_many_range"])
def test_a_range_entry_is_checked_before_anything_is_launched(ctx, fn):
    K = _lib.KIND_FIELD_RANGE
    assert call(ctx, [K], [b"v"], [ENTRY + b"\x00"], fn=fn) == (0, 1, 0)                     # [5, 6]: the first row
    assert call(ctx, [K], [b"v"], [ENTRY + b"\x04"], fn=fn) == (0, 0, 0)                     # (5, 6]
    assert call(ctx, [K], [b"v"], [ENTRY + b"\x0f"], fn=fn) == (0, 3, 0)                     # unbounded on both sides
    assert call(ctx, [0, K], [b"m", b"v"], [b"", ENTRY], fn=fn)[0] == BSG_E_INVALID          # 16 bytes
    assert "condition 1" in last_error(ctx) and "17 bytes" in last_error(ctx)
    assert call(ctx, [K], [b"v"], [ENTRY + b"\x00\x00"], fn=fn)[0] == BSG_E_INVALID          # 18 bytes
    assert call(ctx, [K], [b"v"], [b""], fn=fn)[0] == BSG_E_INVALID
    assert call(ctx, [K], [b"v"], [ENTRY + b"\x10"], fn=fn)[0] == BSG_E_INVALID              # flag bit 4
    assert "condition 0" in last_error(ctx) and "flags" in last_error(ctx)
    assert call(ctx, [K], [b""], [ENTRY + b"\x0f"], fn=fn) == (0, 0, 0)                      # an empty field never holds
    # the text consumers do not share a table with range conditions yet
    for kind, tok in ((_lib.KIND_FIELD_REGEX, b"a.c"), (_lib.KIND_SUBSTRING, b"abc"), (_lib.KIND_FIELD_SUBSTRING, b"abc")):
        assert call(ctx, [K, kind], [b"v", b"m"], [ENTRY + b"\x00", tok], fn=fn)[0] == BSG_E_UNSUPPORTED
        assert "condition 1" in last_error(ctx) and "kind %d" % kind in last_error(ctx)
    assert call(ctx, [7], [b"v"], [ENTRY + b"\x00"], fn=fn)[0] == BSG_E_INVALID and "unknown kind 7" in last_error(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["bsg_match_rows", "bsg_match_rows_regex", "bsg_match_rows_tok", "bsg_match_rows_substr", "bsg_match_rows_regex_substr",
                                "bsg_match_rows_many", "bsg_match_rows_many_regex", "bsg_match_rows_many_substr", "bsg_match_rows_many_regex_substr",
                                "bsg_match_rows_wide", "bsg_match_rows_wide_substr", "bsg_match_rows_lookup", "bsg_match_rows_lookup_regex"])
def test_every_other_entry_point_still_calls_kind_6_unknown(ctx, fn):
    assert call(ctx, [_lib.KIND_FIELD_RANGE], [b"v"], [ENTRY + b"\x00"], fn=fn)[0] == BSG_E_INVALID
    assert "unknown kind 6" in last_error(ctx)
