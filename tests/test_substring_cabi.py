"""The substring calls at the C boundary: a plain C99 program links bsg_match_rows_substr / bsg_match_rows_many_substr and the host
calls; the headers declare them with the argument lists of bsg_match_rows_tok / bsg_match_rows_many; and (on a GPU: every check
of these calls sits behind the context) what they refuse before anything is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q
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
    static const char rows[] = "{\"msg\":\"Connection reset by peer\"}{\"msg\":\"all good\"}";
    const uint64_t row_off[3] = {0, 34, 52};
    static const char conds[] = "ction resmsgGOOD";
    static const char tree[] = "{\"ExpressionType\":\"CONDITION\",\"Condition\":{\"Needle\":\"CTION RES\"}}";
    const uint32_t cond_off[5] = {0, 0, 9, 12, 16}, kinds[2] = {BSG_KIND_SUBSTRING, BSG_KIND_FIELD_SUBSTRING};
    const uint32_t prog[1] = {BSG_OP(BSG_OP_TERM, 0)}, progs[2] = {BSG_OP(BSG_OP_TERM, 0), BSG_OP(BSG_OP_TERM, 1)}, prog_off[3] = {0, 1, 2};
    uint64_t bits[2] = {0, 0};
    uint32_t fb[2], nfb = 7;
    uint8_t *terms = NULL;
    uint64_t terms_len = 0;
    bsg_tokenizer tok;
    bsg_ctx *ctx = NULL;
    int ids[1] = {0};
    int32_t rc;
    /* without a context both calls refuse like every entry point */
    if (bsg_match_rows_substr(NULL, (const uint8_t *)rows, row_off, 2, (const uint8_t *)conds, cond_off, kinds, 2, prog, 1, NULL, bits, fb, 2, &nfb) != BSG_E_INVALID) return 1;
    if (bsg_match_rows_many_substr(NULL, (const uint8_t *)rows, row_off, 2, (const uint8_t *)conds, cond_off, kinds, 2, progs, prog_off, 2, NULL, NULL, 0, NULL, bits,
                                   fb, 2, &nfb) != BSG_E_INVALID) return 2;
    /* the host side needs no device: "timeout" under the trigram spec */
    if (bsg_tokenizer_default(&tok) != BSG_OK) return 3;
    tok.flags |= BSG_TOK_NGRAM(3);
    if (bsh_substring_terms((const uint8_t *)"TimeOut", 7, &tok, &terms, &terms_len) != 0 || terms_len != 5 * 7 || memcmp(terms + 4, "tim", 3) != 0) return 4;
    bsh_free(terms);
    if (bsh_match_row_substring(tree, strlen(tree), (const uint8_t *)rows, 34, NULL) != 1) return 5;
    rc = bsg_open(ids, 1, &ctx);
    printf("open=%d\n", rc);
    if (rc == BSG_OK) {
        if (bsg_match_rows_substr(ctx, (const uint8_t *)rows, row_off, 2, (const uint8_t *)conds, cond_off, kinds, 2, prog, 1, NULL, bits, fb, 2, &nfb) != BSG_OK) return 6;
        if (nfb != 0 || bits[0] != 1) return 7;
        if (bsg_match_rows_many_substr(ctx, (const uint8_t *)rows, row_off, 2, (const uint8_t *)conds, cond_off, kinds, 2, progs, prog_off, 2, NULL, NULL, 0, NULL, bits,
                                       fb, 2, &nfb) != BSG_OK) return 8;
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
    src = tmp_path / "substr_caller.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "substr_caller"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libbloomgpu.so", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    return out.stdout


def test_a_plain_c99_program_links_the_substring_calls(tmp_path):
    out = run_c_caller(tmp_path)
    if _lib.load().bsg_device_count() == 0:
        assert "open=-6" in out


@pytest.mark.gpu
def test_the_c_program_matches_on_the_device(tmp_path):
    assert "matched" in run_c_caller(tmp_path)


def test_the_headers_declare_the_calls_with_their_neighbours_arguments():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    host_h = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()

    def params(name, text):
        m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, text)
        assert m, name
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params("bsg_match_rows_substr", gpu_h) == params("bsg_match_rows_tok", gpu_h)
    assert params("bsg_match_rows_many_substr", gpu_h) == params("bsg_match_rows_many", gpu_h)
    assert "#define BSG_KIND_SUBSTRING        4u" in gpu_h and "#define BSG_KIND_FIELD_SUBSTRING  5u" in gpu_h
    assert len(params("bsh_substring_terms", host_h)) == 5 and len(params("bsh_prune_query_sub", host_h)) == 9
    assert len(params("bsh_match_row_substring", host_h)) == 5
    L = _lib.load()
    Hst.lib()
    for name in ("bsg_match_rows_substr", "bsg_match_rows_many_substr", "bsh_substring_terms", "bsh_prune_query_sub", "bsh_match_row_substring"):
        assert hasattr(L, name) and name in _lib.EXPORTS + Hst.HOST_EXPORTS
    assert (_lib.KIND_SUBSTRING, _lib.KIND_FIELD_SUBSTRING) == (4, 5)
    n = C.c_uint32()
    assert L.bsg_match_rows_substr(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_many_substr(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID


# ---- what the calls refuse before a launch ----
ROWS = [b'{"msg":"abc"}', b'{"msg":"xyz"}']


def call(ctx, kinds, fields, needles, prog=None, fn="bsg_match_rows_substr"):
    """-> the status of one raw call over ROWS (single: the program TERM 0; batched: that one query)"""
    L = ctx.L
    off = np.array([0, len(ROWS[0]), len(ROWS[0]) + len(ROWS[1])], dtype=np.uint64)
    blob = np.frombuffer(b"".join(ROWS), dtype=np.uint8)
    cblob, coff = pack_entries([s for pair in zip(fields, needles) for s in pair])
    kinds = np.asarray(kinds, dtype=np.uint32)
    ops = np.asarray([_lib.op(_lib.OP_TERM, 0)] if prog is None else prog, dtype=np.uint32)
    poff = np.array([0, len(ops)], dtype=np.uint32)
    bits, fb, nfb = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint32), C.c_uint32()
    head = (ctx.h, _lib._ptr(blob), _lib._ptr(off), 2, _lib._ptr(cblob), _lib._ptr(coff), _lib._ptr(kinds), len(kinds), _lib._ptr(ops))
    tail = (_lib._ptr(bits), _lib._ptr(fb), 2, C.byref(nfb))
    if fn in ("bsg_match_rows", "bsg_match_rows_regex"):
        return getattr(L, fn)(*head, len(ops), *tail), bits, nfb.value
    if fn in ("bsg_match_rows_substr", "bsg_match_rows_tok"):
        return getattr(L, fn)(*head, len(ops), None, *tail), bits, nfb.value
    return getattr(L, fn)(*head, poff.ctypes.data, 1, None, None, 0, None, *tail), bits, nfb.value


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["bsg_match_rows_substr", "bsg_match_rows_many_substr"])
def test_needles_are_checked_before_anything_is_launched(ctx, fn):
    K = _lib.KIND_SUBSTRING
    assert call(ctx, [K], [b""], [b""], fn=fn)[0] == BSG_E_INVALID                          # an empty needle
    assert call(ctx, [K], [b""], [b"ab\xff"], fn=fn)[0] == BSG_E_INVALID                    # invalid UTF-8
    assert call(ctx, [K], [b""], [b"\xc3"], fn=fn)[0] == BSG_E_INVALID                      # a cut-off rune
    assert call(ctx, [K], [b""], [b"a" * 64], fn=fn)[0] == 0
    assert call(ctx, [K], [b""], [b"a" * 65], fn=fn)[0] == BSG_E_UNSUPPORTED                # 65 folded bytes
    assert "65 bytes" in ctx.L.bsg_last_error(ctx.h).decode()
    # U+212A is 3 bytes raw and 1 folded: 64 of them fold to 64 bytes
    assert call(ctx, [K], [b""], ["K".encode() * 64], fn=fn)[0] == 0
    assert call(ctx, [K], [b""], ["K".encode() * 65], fn=fn)[0] == BSG_E_UNSUPPORTED
    # two 64-byte needles fill both words; a third needle of one byte has no room
    rc, bits, nfb = call(ctx, [K, K], [b"", b""], [b"a" * 64, b"b" * 64], fn=fn)
    assert (rc, int(bits[0]), nfb) == (0, 0, 0)
    assert call(ctx, [K, K, K], [b"", b"", b""], [b"a" * 64, b"b" * 64, b"c"], fn=fn)[0] == BSG_E_UNSUPPORTED
    assert call(ctx, [K, K, K], [b"", b"", b""], [b"a" * 40, b"b" * 40, b"c" * 40], fn=fn)[0] == BSG_E_UNSUPPORTED      # 40 + 40 straddles
    rc, bits, nfb = call(ctx, [K, K, K], [b"", b"", b""], [b"bc", b"b" * 60, b"c" * 60], fn=fn)
    assert (rc, int(bits[0]), nfb) == (0, 1, 0)
    # FieldRegex conditions do not share a call with substring conditions yet
    assert call(ctx, [K, _lib.KIND_FIELD_REGEX], [b"", b"msg"], [b"abc", b"a.c"], fn=fn)[0] == BSG_E_UNSUPPORTED
    assert "regex and substring" in ctx.L.bsg_last_error(ctx.h).decode()
    assert call(ctx, [6], [b""], [b"abc"], fn=fn)[0] == BSG_E_INVALID and "unknown kind" in ctx.L.bsg_last_error(ctx.h).decode()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["bsg_match_rows", "bsg_match_rows_regex", "bsg_match_rows_tok", "bsg_match_rows_many", "bsg_match_rows_many_regex"])
@pytest.mark.parametrize("kind", [4, 5])
def test_every_other_entry_point_still_calls_the_new_kinds_unknown(ctx, fn, kind):
    assert call(ctx, [kind], [b"msg"], [b"abc"], fn=fn)[0] == BSG_E_INVALID
    assert "unknown kind %d" % kind in ctx.L.bsg_last_error(ctx.h).decode()
