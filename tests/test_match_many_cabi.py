"""The batched row matcher's surface without a GPU: the headers declare bsg_match_rows_many / bse_query_many, the built library
exports them, the ctypes layer binds them, query.CompiledMatcherBatch deduplicates conditions across queries and keeps each
query's program (CompiledMatcher's, indices remapped), its limits raise, and the Go binding's calls agree with the header."""
import os
import re
import subprocess
import sys

import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headers_declare_and_the_library_exports_the_batched_calls():
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    host_h = open(os.path.join(ROOT, "include", "bloomsearch_host.h")).read()
    m = re.search(r"BSG_API int32_t bsg_match_rows_many\(([^;]*)\);", gpu_h)
    assert m, "bloomgpu.h does not declare bsg_match_rows_many"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["ctx", "rows", "row_off", "n_rows", "cond_bytes", "cond_off", "cond_kinds", "n_conds", "prog_ops", "prog_off", "n_queries",
                     "set_first_row", "query_mask_of_set", "n_sets", "tok", "out_bits", "out_fallback_rows", "fallback_cap", "out_n_fallback"]
    assert re.search(r"BSG_API int32_t bse_query_many\(bse_engine \*e, const char \*queries_json, uint64_t len, char \*\*out_json, uint64_t \*out_len\);", host_h)
    assert "bsg_match_rows_many" in _lib.EXPORTS and "bse_query_many" in Hst.HOST_EXPORTS
    L = _lib.load()
    assert hasattr(L, "bsg_match_rows_many") and hasattr(L, "bse_query_many")
    assert len(L.bsg_match_rows_many.argtypes) == len(names)
    Hst.lib()
    assert len(L.bse_query_many.argtypes) == 5


def test_calls_refuse_bad_arguments_before_touching_a_device():
    L = _lib.load()
    import ctypes as C
    n = C.c_uint32()
    # a null context is refused like every other entry point's; the host call refuses a null engine
    assert L.bsg_match_rows_many(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, 0, None, None, None, 0, C.byref(n)) == _lib.BSG_E_INVALID
    Hst.lib()
    p, ln = C.c_void_p(), C.c_uint64()
    assert L.bse_query_many(None, b"[]", 2, C.byref(p), C.byref(ln)) == -1


def test_compiled_matcher_batch_dedups_conditions_and_keeps_programs():
    shared = Q.FieldToken("service", "payment")
    exprs = [Q.And(Q.FieldToken("level", "error"), shared), Q.Or(shared, Q.Token("timeout"), Q.Field("nested.az")), None, Q.And(), shared,
             Q.Or(Q.Token("payment"), Q.Field("service"), Q.FieldToken("service", "Payment"))]
    b = Q.CompiledMatcherBatch(exprs)
    assert b.n_queries == len(exprs) and b.prog_off[0] == 0 and len(b.prog_off) == len(exprs) + 1
    table = list(zip(b.kinds, b.fields, b.tokens))
    assert len(set(table)) == len(table)                                           # distinct
    assert table.count((_lib.KIND_FIELD_TOKEN, b"service", b"payment")) == 1       # shared by queries 0, 1 and 4
    # same strings under another kind, and another spelling, are other conditions
    assert (_lib.KIND_TOKEN, b"", b"payment") in table and (_lib.KIND_FIELD, b"service", b"") in table
    assert (_lib.KIND_FIELD_TOKEN, b"service", b"Payment") in table
    assert len(table) == 7
    for q, e in enumerate(exprs):
        one = Q.CompiledMatcher(e)
        prog = b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]]
        assert len(prog) == len(one.prog_ops)
        for got, want in zip(prog, one.prog_ops):
            assert got >> 28 == want >> 28
            if want >> 28 == _lib.OP_TERM:
                i, j = got & 0x0FFFFFFF, want & 0x0FFFFFFF
                assert table[i] == (one.kinds[j], one.fields[j], one.tokens[j]) and b.index_maps[q][j] == i
            else:
                assert got == want
    assert b.prog_off[3] == b.prog_off[2]                                          # the nil expression: an empty program
    assert Q.CompiledMatcherBatch([]).n_queries == 0


def test_compiled_matcher_batch_limits_raise():
    ok = Q.CompiledMatcherBatch([Q.Token("t%d" % (i % 64)) for i in range(64)])
    assert ok.n_queries == 64 and len(ok.kinds) == 64
    with pytest.raises(ValueError):
        Q.CompiledMatcherBatch([Q.Token("t")] * 65)                                # 65 queries
    with pytest.raises(ValueError):
        Q.CompiledMatcherBatch([Q.Token("t%d" % i) for i in range(33)] + [Q.Field("f%d" % i) for i in range(32)])   # 65 distinct conditions
    with pytest.raises(ValueError):
        Q.CompiledMatcherBatch([Q.And(*[Q.Token("t%d" % i) for i in range(65)])])  # ... in one query
    # ops over the cap: 64 conditions per query lower to 64 terms + 63 binary ops; 17 such queries exceed 2 048
    big = Q.And(*[Q.Token("t%d" % i) for i in range(64)])
    assert Q.lowered_ops(Q.CompiledMatcher(big).prog_ops) == 127
    Q.CompiledMatcherBatch([big] * 16)
    with pytest.raises(ValueError):
        Q.CompiledMatcherBatch([big] * 17)
    assert Q.lowered_ops(Q.CompiledMatcher(Q.Or(Q.And(), Q.Or(Q.Token("a")))).prog_ops) == 3      # TRUE, TERM, one binary OR


def test_go_binding_is_clean_with_the_new_file():
    assert os.path.exists(os.path.join(ROOT, "go", "bloomgpu", "match_many_test.go"))
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsMany(" in src and "C.bsg_match_rows_many(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
