"""bsg_match_rows_lookup / bsg_match_rows_lookup_rows' surface without a GPU: the header declares them with exactly the arguments of the
two wide calls, the built library exports them, ctypes binds them with matching arity, a null context is refused before anything
else, CompiledLookupBatch holds 1 024 distinct conditions and refuses the 1 025th and any FieldRegex condition (validation only: no
device is asked), the 65-condition refusal of CompiledWideBatch still holds, and the Go binding agrees with the header."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from bloomsearch_amd import _lib, query as Q
from tests.test_match_wide_cabi import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_ctypes_agree():
    assert declared("bsg_match_rows_lookup") == declared("bsg_match_rows_wide")
    assert declared("bsg_match_rows_lookup_rows") == declared("bsg_match_rows_wide_rows")
    assert "bsg_match_rows_lookup" in _lib.EXPORTS and "bsg_match_rows_lookup_rows" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.bsg_match_rows_lookup.argtypes) == 20 and len(L.bsg_match_rows_lookup_rows.argtypes) == 24
    n, length = C.c_uint32(), C.c_uint64(7)
    assert L.bsg_match_rows_lookup(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                   C.byref(n)) == _lib.BSG_E_INVALID
    assert b"ctx" in L.bsg_last_error(None)
    assert L.bsg_match_rows_lookup_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                        C.byref(length), None, 0, C.byref(n)) == _lib.BSG_E_INVALID
    assert b"ctx" in L.bsg_last_error(None) and length.value == 7                      # refused before anything is written
    hdr = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert "#define BSG_MATCH_LOOKUP_MAX_CONDS 1024u" in hdr and Q.MATCH_LOOKUP_MAX_CONDS == 1024


def test_compiled_lookup_batch_limits():
    exprs = [Q.Token("t%d" % i) for i in range(512)] + [Q.FieldToken("f%d" % i, "t%d" % i) for i in range(511)] + [Q.Field("f0")]
    b = Q.CompiledLookupBatch(exprs + exprs[:10] + [None, Q.And(exprs[0], exprs[1023])])   # repeated conditions are one table entry
    assert len(b.kinds) == 1024 and b.n_queries == 1036 and sorted(set(b.kinds)) == [_lib.KIND_FIELD, _lib.KIND_TOKEN, _lib.KIND_FIELD_TOKEN]
    assert b.prog_ops[b.prog_off[1035]: b.prog_off[1036]] == [_lib.op(_lib.OP_TERM, 0), _lib.op(_lib.OP_TERM, 1023), _lib.op(_lib.OP_AND, 2)]
    with pytest.raises(ValueError, match="1024 distinct conditions"):
        Q.CompiledLookupBatch(exprs + [Q.Token("one more")])
    with pytest.raises(ValueError, match="FieldRegex"):
        Q.CompiledLookupBatch([Q.Token("a"), (Q.Token("b"), Q.FieldRegex("service", "^pay"))])
    with pytest.raises(ValueError, match="FieldRegex"):
        Q.CompiledLookupBatch([(None, Q.FieldRegex("service", "^pay"))])
    assert Q.CompiledLookupBatch([(Q.Token("b"), None)]).kinds == [_lib.KIND_TOKEN]    # a pair without a regex side is a plain query
    with pytest.raises(ValueError, match="64 distinct conditions"):                    # the wide batch keeps its limit
        Q.CompiledWideBatch(exprs[:65])


def test_go_binding_has_the_lookup_calls():
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsLookup(" in src and "func (g *Context) MatchRowsLookupRows(" in src
    assert "C.bsg_match_rows_lookup(" in src and "C.bsg_match_rows_lookup_rows(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
