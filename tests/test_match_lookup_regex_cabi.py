"""bsg_match_rows_lookup_regex / bsg_match_rows_lookup_regex_rows' surface without a GPU: the header declares them with exactly the
arguments of the two wide calls, the built library exports them, ctypes binds them with the wide calls' argtypes, a null context is
refused before anything else, CompiledLookupRegexBatch holds 1 008 + 16 conditions and refuses the 1 025th condition and the 17th
regex condition (validation only: no device is asked), CompiledLookupBatch still refuses regex, and the Go binding agrees with the
header."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from bloomsearch_amd import _lib, query as Q
from tests.test_match_wide_cabi import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_ctypes_agree():
    assert declared("bsg_match_rows_lookup_regex") == declared("bsg_match_rows_wide")
    assert declared("bsg_match_rows_lookup_regex_rows") == declared("bsg_match_rows_wide_rows")
    assert "bsg_match_rows_lookup_regex" in _lib.EXPORTS and "bsg_match_rows_lookup_regex_rows" in _lib.EXPORTS
    L = _lib.load()
    assert L.bsg_match_rows_lookup_regex.argtypes == L.bsg_match_rows_wide.argtypes and len(L.bsg_match_rows_lookup_regex.argtypes) == 20
    assert L.bsg_match_rows_lookup_regex_rows.argtypes == L.bsg_match_rows_wide_rows.argtypes and len(L.bsg_match_rows_lookup_regex_rows.argtypes) == 24
    n, length = C.c_uint32(), C.c_uint64(7)
    assert L.bsg_match_rows_lookup_regex(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                         C.byref(n)) == _lib.BSG_E_INVALID
    assert b"ctx" in L.bsg_last_error(None)
    assert L.bsg_match_rows_lookup_regex_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                              C.byref(length), None, 0, C.byref(n)) == _lib.BSG_E_INVALID
    assert b"ctx" in L.bsg_last_error(None) and length.value == 7                      # refused before anything is written


def test_compiled_lookup_regex_batch_limits():
    tokens = [Q.Token("t%d" % i) for i in range(1008)]
    regexes = [(None, Q.FieldRegex("r%d" % i, "x|y")) for i in range(16)]
    b = Q.CompiledLookupRegexBatch(tokens + regexes + tokens[:5] + regexes[:5] + [(Q.And(tokens[0], tokens[1007]), Q.FieldRegex("r15", "x|y"))])
    assert len(b.kinds) == 1024 and b.n_queries == 1035 and b.kinds.count(_lib.KIND_FIELD_REGEX) == 16   # repeated conditions are one table entry
    assert b.kinds[1008:] == [_lib.KIND_FIELD_REGEX] * 16 and b.fields[1023] == b"r15" and b.tokens[1023] == b"x|y"
    assert _lib.op(_lib.OP_TERM, 1023) in b.prog_ops[b.prog_off[1034]: b.prog_off[1035]]
    with pytest.raises(ValueError, match="1024 distinct conditions"):
        Q.CompiledLookupRegexBatch(tokens + regexes + [Q.Token("one more")])
    with pytest.raises(ValueError, match="16 distinct regex conditions"):
        Q.CompiledLookupRegexBatch(tokens[:10] + regexes + [(None, Q.FieldRegex("r16", "x|y"))])
    with pytest.raises(ValueError, match="16 distinct regex conditions"):              # the same field under another pattern is another condition
        Q.CompiledLookupRegexBatch(regexes + [(Q.Token("a"), Q.FieldRegex("r0", "y|x"))])
    assert Q.CompiledLookupRegexBatch(tokens[:200]).kinds == [_lib.KIND_TOKEN] * 200   # a regex-free batch is a plain lookup table


def test_compiled_lookup_batch_still_refuses_regex():
    with pytest.raises(ValueError, match="FieldRegex"):
        Q.CompiledLookupBatch([Q.Token("a"), (Q.Token("b"), Q.FieldRegex("service", "^pay"))])
    with pytest.raises(ValueError, match="FieldRegex"):
        Q.CompiledLookupBatch([(None, Q.FieldRegex("service", "^pay"))])


def test_go_binding_has_the_lookup_regex_calls():
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsLookupRegex(" in src and "func (g *Context) MatchRowsLookupRegexRows(" in src
    assert "C.bsg_match_rows_lookup_regex(" in src and "C.bsg_match_rows_lookup_regex_rows(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
