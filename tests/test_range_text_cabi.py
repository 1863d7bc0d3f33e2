"""bsg_match_rows_regex_substr_range / bsg_match_rows_many_regex_substr_range at the C boundary: the header declares them with their
parents' parameter lists, the library exports them, a plain C99 program links them, query.CompiledRowTextRangeQuery lowers the four
sides, the literal bits of tests/range_text_cases.EDGES are what the restatements say — and, where a device is present, every refusal
comes before any launch while every other entry point answers kinds 3-6 as before."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID, BSG_E_UNSUPPORTED, OP_AND, OP_FALSE, OP_TERM, OP_TRUE, op
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests.test_range_cabi import ENTRY, call, last_error
from tests.test_regex_substr_cabi import constant, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
NEW = ("bsg_match_rows_regex_substr_range", "bsg_match_rows_many_regex_substr_range")


def test_the_header_declares_both_calls_with_their_parents_parameters():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert params(NEW[0], gpu_h) == params("bsg_match_rows_regex_substr", gpu_h) and len(params(NEW[0], gpu_h)) == 15
    assert params(NEW[1], gpu_h) == params("bsg_match_rows_many", gpu_h) and len(params(NEW[1], gpu_h)) == 19


def test_the_library_exports_them():
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS
    n = C.c_uint32()
    # without a context both refuse like every entry point
    assert L.bsg_match_rows_regex_substr_range(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, C.byref(n)) == BSG_E_INVALID
    assert L.bsg_match_rows_many_regex_substr_range(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0,
                                                    C.byref(n)) == BSG_E_INVALID


C_PROGRAM = r"""
/* A plain C99 caller of the two calls: without a context both answer BSG_E_INVALID. */
#include <stdio.h>
#include "bloomgpu.h"

int main(void)
{
    uint32_t n = 0;
    int32_t a = bsg_match_rows_regex_substr_range(NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, 0, &n);
    int32_t b = bsg_match_rows_many_regex_substr_range(NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL, 0, NULL, NULL, NULL, 0, &n);
    printf("single=%d many=%d kind=%u entry=%u\n", (int)a, (int)b, (unsigned)BSG_KIND_FIELD_RANGE, (unsigned)BSG_RANGE_ENTRY_BYTES);
    return a == BSG_E_INVALID && b == BSG_E_INVALID ? 0 : 1;
}
"""


def test_a_plain_c99_program_links_them(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    _lib.load()
    src, exe, libdir = tmp_path / "caller.c", tmp_path / "caller", os.path.dirname(_lib.LIB_PATH)
    src.write_text(C_PROGRAM)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libbloomgpu.so", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "single=%d many=%d kind=6 entry=17" % (BSG_E_INVALID, BSG_E_INVALID) in out.stdout, (out.stdout, out.stderr)


def test_compiled_row_text_range_query_is_and_of_the_four_sides():
    m = Q.CompiledRowTextRangeQuery(Q.FieldToken("lvl", "error"), Q.FieldRegex("msg", "timeout$"), Q.Substring("10.0.3."), Q.FieldRange("ts", 5, None, lo_open=True))
    assert m.kinds == [_lib.KIND_FIELD_TOKEN, _lib.KIND_FIELD_REGEX, _lib.KIND_SUBSTRING, _lib.KIND_FIELD_RANGE]
    assert m.fields == [b"lvl", b"msg", b"", b"ts"] and m.tokens[:3] == [b"error", b"timeout$", b"10.0.3."]
    assert m.tokens[3] == (5).to_bytes(8, "little") + bytes(8) + bytes([_lib.RANGE_NO_HI | _lib.RANGE_LO_OPEN])
    assert m.prog_ops == [op(OP_TERM, 0), op(OP_TERM, 1), op(OP_TERM, 2), op(OP_TERM, 3), op(OP_AND, 4)]
    # each missing side is TRUE, as in the parents
    assert Q.CompiledRowTextRangeQuery(None, None, None, None).prog_ops == [op(OP_TRUE)] * 4 + [op(OP_AND, 4)]
    # an empty Or is FALSE, an empty And TRUE, an empty range or regex field FALSE, as in the parents
    m = Q.CompiledRowTextRangeQuery(None, Q.RegexAnd(), Q.FieldSubstring("a", "x"), Q.RangeOr())
    assert m.prog_ops == [op(OP_TRUE), op(OP_TRUE), op(OP_TERM, 0), op(OP_FALSE), op(OP_AND, 4)] and m.kinds == [_lib.KIND_FIELD_SUBSTRING]
    m = Q.CompiledRowTextRangeQuery(None, Q.FieldRegex("", "x"), None, Q.FieldRange("", 1, 2))
    assert m.prog_ops == [op(OP_TRUE), op(OP_FALSE), op(OP_TRUE), op(OP_FALSE), op(OP_AND, 4)] and m.kinds == []
    b = Q.CompiledRowTextRangeQueryBatch([(None, Q.FieldRegex("m", "x"), None, Q.FieldRange("v", 1, 2)), (None, None, Q.Substring("x"), Q.FieldRange("v", 1, 2)),
                                          (None, None, None, Q.FieldRange("v", 1, 2, hi_open=True))])
    assert b.n_queries == 3 and b.kinds == [_lib.KIND_FIELD_REGEX, _lib.KIND_FIELD_RANGE, _lib.KIND_SUBSTRING, _lib.KIND_FIELD_RANGE]   # a range condition is distinct by its bounds and flags


@pytest.mark.parametrize("walker", RT.WALKERS)
def test_the_literal_bits_of_the_edge_cases_are_the_restatements(walker):
    RT.check_edges_against_the_restatements(SR.WALKERS[walker])
    rows, blooms, regexes, subs, ranges = RT.full_table()
    m, sides = RT.table(regexes, subs, ranges, blooms)
    sat = RT.sat_columns(rows, sides, SR.WALKERS[walker])
    assert len(m.kinds) == 64 and all(0 < c.sum() < len(rows) for c in sat)


def test_the_three_consumer_instances_add_no_lds():
    """the instances launch with the regex_substr instances' bytes: the needle table, then a blob under the caps that table leaves"""
    text = open(os.path.join(CSRC, "ingest.hip.h")).read() + open(os.path.join(CSRC, "match.hip.h")).read()
    assert constant(text, "kRxSubLdsCap") == RT.SINGLE_CAP == 80 * 1024 - constant(text, "kMatchSubLdsBytes")
    assert constant(text, "kRxManySubLdsCap") == RT.MANY_CAP == 80 * 1024 - constant(text, "kMatchManySubLdsBytes")
    body = open(os.path.join(CSRC, "match.hip.h")).read()
    for name in ("k_match_rows_regex_substr_range", "k_match_rows_many_regex_substr_range"):
        for suffix in ("", "_tok", "_gram"):
            assert re.search(r"void %s%s\(" % (name, suffix), body), name + suffix
    # the three-consumer slots hold these kernels, and every slot with the substring consumer launches with the needle table's bytes
    api, route = open(os.path.join(CSRC, "match_api.inc")).read(), open(os.path.join(CSRC, "host", "match_route.hpp")).read()
    for mode, name in (("Single", "k_match_rows_regex_substr_range"), ("Many", "k_match_rows_many_regex_substr_range")):
        for suffix, tok in (("", "Default"), ("_tok", "Spec"), ("_gram", "Gram")):
            assert re.search(r"X\(%s, RegexSubstrRange, %s, %s%s\)" % (mode, tok, name, suffix), route), name + suffix
    assert re.search(r"has_substr\(Consumers c\) \{ return [^}]*c == Consumers::RegexSubstrRange; \}", route)
    assert "case bsh_route::Mode::Single: return sub ? bsg::kMatchSubLdsBytes : bsg::kMatchLdsBytes;" in api
    assert "case bsh_route::Mode::Many: return sub ? bsg::kMatchManySubLdsBytes : bsg::kMatchManyLdsBytes;" in api


# ---- with a device: what the two calls refuse before a launch, and what the other entry points still answer ----
K_RX, K_SUB, K_FSUB, K_RNG = _lib.KIND_FIELD_REGEX, _lib.KIND_SUBSTRING, _lib.KIND_FIELD_SUBSTRING, _lib.KIND_FIELD_RANGE
E0 = ENTRY + b"\x00"                                           # [5, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("fn", NEW)
def test_every_kind_keeps_its_entry_format_and_refusals(ctx, fn):
    before = int(ctx.device_calls().sum())
    bad = [
        ([K_RNG, K_SUB], [b"v", b""], [ENTRY, b"abc"], BSG_E_INVALID, ("condition 0", "17 bytes")),                  # 16 bytes
        ([K_SUB, K_RNG], [b"", b"v"], [b"abc", ENTRY + b"\x10"], BSG_E_INVALID, ("condition 1", "flags")),           # flag bit 4
        ([K_RNG, K_SUB], [b"v", b""], [E0, b""], BSG_E_INVALID, ("condition 1", "needle")),                          # an empty needle
        ([K_RNG, K_FSUB], [b"v", b"m"], [E0, b"\xff\xfe"], BSG_E_INVALID, ("condition 1", "needle")),                # invalid UTF-8
        ([K_RNG, K_SUB], [b"v", b""], [E0, b"a" * 65], BSG_E_UNSUPPORTED, ("condition 1", "65 bytes")),              # a needle over 64 folded bytes
        ([K_RNG, K_SUB, K_SUB, K_SUB], [b"v", b"", b"", b""], [E0, b"a" * 40, b"b" * 40, b"c" * 40], BSG_E_UNSUPPORTED, ("needles",)),
        ([K_RNG, K_RX], [b"v", b"m"], [E0, b"\\bx"], BSG_E_UNSUPPORTED, ("regex condition 1",)),                     # outside the compiler's subset
        ([K_RNG] + [K_RX] * 17, [b"v"] + [b"m"] * 17, [E0] + [b"x%d" % i for i in range(17)], BSG_E_UNSUPPORTED, ("17 regex conditions",)),
        ([K_RNG] + [K_SUB] * 64, [b"v"] + [b""] * 64, [E0] + [b"x"] * 64, BSG_E_UNSUPPORTED, ("65 conditions",)),
        ([K_RNG, K_SUB, 7], [b"v", b"", b"m"], [E0, b"abc", b"x"], BSG_E_INVALID, ("condition 2", "unknown kind 7")),
        ([7], [b"v"], [E0], BSG_E_INVALID, ("condition 0", "unknown kind 7")),
    ]
    for kinds, fields, tokens, code, words in bad:
        assert call(ctx, kinds, fields, tokens, fn=fn)[0] == code, (kinds, last_error(ctx))
        assert all(w in last_error(ctx) for w in words), last_error(ctx)
    assert int(ctx.device_calls().sum()) == before                # nothing was launched
    # and what passes: rows {"v":5,"m":"abc"} and {"v":7} under the program TERM 0
    assert call(ctx, [K_RNG, K_SUB], [b"v", b""], [E0, b"abc"], fn=fn) == (0, 1, 0)
    assert call(ctx, [K_SUB, K_RNG], [b"", b"v"], [b"7", ENTRY + b"\x0f"], fn=fn) == (0, 2, 0)         # the needle reads the number's text
    assert call(ctx, [K_RX, K_RNG], [b"m", b"v"], [b"a.c", E0], fn=fn) == (0, 1, 0)
    assert call(ctx, [K_FSUB, K_RX, K_RNG], [b"m", b"v", b"v"], [b"bc", b"^7$", E0], fn=fn) == (0, 1, 0)
    assert call(ctx, [K_RNG], [b"v"], [ENTRY + b"\x04"], fn=fn) == (0, 0, 0)                            # (5, 6]: the range call's path
    assert call(ctx, [K_RX, K_SUB], [b"m", b""], [b"a.c", b"abc"], fn=fn) == (0, 1, 0)                  # the regex_substr call's path
    assert int(ctx.device_calls().sum()) == before + 6


OTHERS = ["bsg_match_rows", "bsg_match_rows_regex", "bsg_match_rows_tok", "bsg_match_rows_substr", "bsg_match_rows_regex_substr", "bsg_match_rows_range",
          "bsg_match_rows_many", "bsg_match_rows_many_regex", "bsg_match_rows_many_substr", "bsg_match_rows_many_regex_substr", "bsg_match_rows_many_range",
          "bsg_match_rows_wide", "bsg_match_rows_wide_substr", "bsg_match_rows_wide_range", "bsg_match_rows_lookup", "bsg_match_rows_lookup_regex"]
RANGE_CALLS = ("bsg_match_rows_range", "bsg_match_rows_many_range", "bsg_match_rows_wide_range")
# (kind, entry, the calls that take it); every other call of OTHERS refuses it
TAKES = {K_RX: ("bsg_match_rows_regex", "bsg_match_rows_tok", "bsg_match_rows_regex_substr", "bsg_match_rows_many_regex", "bsg_match_rows_many_regex_substr",
                "bsg_match_rows_wide", "bsg_match_rows_wide_substr", "bsg_match_rows_lookup_regex"),
         K_SUB: ("bsg_match_rows_substr", "bsg_match_rows_regex_substr", "bsg_match_rows_many_substr", "bsg_match_rows_many_regex_substr", "bsg_match_rows_wide_substr"),
         K_RNG: RANGE_CALLS}
TAKES[K_FSUB] = TAKES[K_SUB]


@pytest.mark.gpu
@pytest.mark.parametrize("fn", OTHERS)
def test_every_existing_entry_point_answers_kinds_3_to_6_as_before(ctx, fn):
    for kind, field, entry in ((K_RX, b"m", b"a.c"), (K_SUB, b"", b"abc"), (K_FSUB, b"m", b"abc"), (K_RNG, b"v", E0)):
        status = call(ctx, [kind], [field], [entry], fn=fn)[0]
        if fn in TAKES[kind]:
            assert status == 0, (fn, kind, last_error(ctx))
        elif kind == K_RNG:
            assert status == BSG_E_INVALID and "unknown kind 6" in last_error(ctx), (fn, last_error(ctx))
        elif fn in RANGE_CALLS:
            assert status == BSG_E_UNSUPPORTED and "kind %d" % kind in last_error(ctx), (fn, kind, last_error(ctx))
        elif kind == K_RX and fn == "bsg_match_rows":
            assert status == BSG_E_INVALID and "unknown kind 3" in last_error(ctx), last_error(ctx)
        elif kind == K_RX:
            assert status == BSG_E_UNSUPPORTED and "FieldRegex" in last_error(ctx), (fn, last_error(ctx))       # a call sized without the DFAs says so
        else:
            assert status == BSG_E_INVALID and "unknown kind %d" % kind in last_error(ctx), (fn, kind, last_error(ctx))
    # a range condition beside a text condition: the range calls name the text condition, every other call the range one
    status = call(ctx, [K_RNG, K_SUB], [b"v", b""], [E0, b"abc"], fn=fn)[0]
    assert status == (BSG_E_UNSUPPORTED if fn in RANGE_CALLS else BSG_E_INVALID), (fn, last_error(ctx))
