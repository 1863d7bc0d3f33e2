"""The batched regex row matcher's surface without a GPU: bloomgpu.h declares bsg_match_rows_many_regex with bsg_match_rows_many's
nineteen parameters, the built library exports it and the ctypes layer binds it, a null context is refused,
query.CompiledRowQueryBatch deduplicates conditions across queries and keeps each query's program (CompiledRowQuery's, indices
remapped), its limits raise, and the Go binding's calls agree with the header."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from bloomsearch_amd import _lib, query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ctx", "rows", "row_off", "n_rows", "cond_bytes", "cond_off", "cond_kinds", "n_conds", "prog_ops", "prog_off", "n_queries",
         "set_first_row", "query_mask_of_set", "n_sets", "tok", "out_bits", "out_fallback_rows", "fallback_cap", "out_n_fallback"]


def declared(header, name):
    m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, header)
    assert m, "bloomgpu.h does not declare " + name
    return [p.strip() for p in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_and_the_library_exports_the_call():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    params = declared(gpu_h, "bsg_match_rows_many_regex")
    assert [re.split(r"[ *]", p)[-1] for p in params] == NAMES
    assert [re.sub(r"\s+", " ", p) for p in params] == [re.sub(r"\s+", " ", p) for p in declared(gpu_h, "bsg_match_rows_many")]   # types and order too
    assert "bsg_match_rows_many_regex" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "bsg_match_rows_many_regex")
    assert len(L.bsg_match_rows_many_regex.argtypes) == 19
    assert list(L.bsg_match_rows_many_regex.argtypes) == list(L.bsg_match_rows_many.argtypes)


def test_a_null_context_is_refused_before_touching_a_device():
    L = _lib.load()
    n = C.c_uint32()
    assert L.bsg_match_rows_many_regex(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0,
                                       C.byref(n)) == _lib.BSG_E_INVALID


def test_compiled_row_query_batch_dedups_conditions_and_keeps_programs():
    shared = Q.FieldRegex("message", "timeout|cache")
    pairs = [(Q.FieldToken("level", "error"), shared),
             (None, Q.RegexOr(shared, Q.FieldRegex("service", "^pay"))),
             (Q.FieldToken("level", "error"), None),
             (None, None),
             (Q.Token("timeout"), Q.RegexAnd(Q.FieldRegex("message", "^pay"), Q.FieldRegex("", "x"), Q.RegexOr())),
             (Q.Field("message"), Q.FieldRegex("message", "timeout|cache"))]
    b = Q.CompiledRowQueryBatch(pairs)
    assert b.n_queries == len(pairs) and b.prog_off[0] == 0 and len(b.prog_off) == len(pairs) + 1
    table = list(zip(b.kinds, b.fields, b.tokens))
    assert len(set(table)) == len(table)
    assert table.count((_lib.KIND_FIELD_REGEX, b"message", b"timeout|cache")) == 1         # shared by queries 0, 1 and 5
    assert table.count((_lib.KIND_FIELD_TOKEN, b"level", b"error")) == 1                   # shared by queries 0 and 2
    # the same pattern on another field and another pattern on the same field are other conditions
    assert (_lib.KIND_FIELD_REGEX, b"service", b"^pay") in table and (_lib.KIND_FIELD_REGEX, b"message", b"^pay") in table
    assert len(table) == 6 and b.kinds.count(_lib.KIND_FIELD_REGEX) == 3
    for q, pair in enumerate(pairs):
        one = Q.CompiledRowQuery(*pair)
        prog = b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]]
        assert len(prog) == len(one.prog_ops)
        for got, want in zip(prog, one.prog_ops):
            assert got >> 28 == want >> 28
            if want >> 28 == _lib.OP_TERM:
                i, j = got & 0x0FFFFFFF, want & 0x0FFFFFFF
                assert table[i] == (one.kinds[j], one.fields[j], one.tokens[j]) and b.index_maps[q][j] == i
            else:
                assert got == want
        assert prog[-1] == _lib.op(_lib.OP_AND, 2)                                         # And(bloom root | TRUE, regex root)
    assert Q.CompiledRowQueryBatch([]).n_queries == 0
    # the plain batch is what it was: no regex side, an empty program for the nil expression
    plain = Q.CompiledMatcherBatch([Q.Token("a"), None])
    assert plain.prog_off == [0, 1, 1] and plain.kinds == [_lib.KIND_TOKEN]


def test_compiled_row_query_batch_limits_raise():
    ok = Q.CompiledRowQueryBatch([(Q.Token("t%d" % i), None) for i in range(64)])
    assert ok.n_queries == 64 and len(ok.kinds) == 64
    with pytest.raises(ValueError):
        Q.CompiledRowQueryBatch([(Q.Token("t"), None)] * 65)                               # 65 queries
    with pytest.raises(ValueError):                                                        # 65 distinct conditions, 16 of them regex
        Q.CompiledRowQueryBatch([(Q.Token("t%d" % i), None) for i in range(49)] + [(None, Q.FieldRegex("f", "x%d" % i)) for i in range(16)])
    sixteen = [(None, Q.FieldRegex("f%d" % i, "x")) for i in range(16)]
    assert Q.CompiledRowQueryBatch(sixteen + sixteen[:3]).kinds.count(_lib.KIND_FIELD_REGEX) == 16     # a repeated one is not a new one
    with pytest.raises(ValueError):
        Q.CompiledRowQueryBatch(sixteen + [(None, Q.FieldRegex("f16", "x"))])              # 17 regex conditions
    with pytest.raises(ValueError):
        Q.CompiledRowQueryBatch([(None, Q.RegexOr(*[Q.FieldRegex("f", "x%d" % i) for i in range(17)]))])   # ... in one query
    big = Q.And(*[Q.Token("t%d" % i) for i in range(64)])                                  # 127 lowered ops, + TRUE and AND per query = 129
    Q.CompiledRowQueryBatch([(big, None)] * 15)
    with pytest.raises(ValueError):
        Q.CompiledRowQueryBatch([(big, None)] * 16)                                        # 16 * 129 = 2 064 > 2 048


def test_go_binding_is_clean_with_the_new_file():
    assert os.path.exists(os.path.join(ROOT, "go", "bloomgpu", "match_many_regex_test.go"))
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsManyRegex(" in src and "C.bsg_match_rows_many_regex(" in src
    assert "func (g *Context) MatchRowsMany(" in src and "C.bsg_match_rows_many(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
