"""bsg_match_rows_wide's surface without a GPU: the header declares bsg_match_rows_wide / bsg_match_wide_size with the documented
argument names, the built library exports them, ctypes binds them with matching arity, a null context is refused,
bsg_match_wide_size (host arithmetic, no context) equals a restatement of the layout and refuses every malformed set table,
query.CompiledWideBatch compiles 300 queries into one table with CompiledMatcher's programs, and the Go binding agrees with the header."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(name):
    gpu_h = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    m = re.search(r"BSG_API int32_t %s\(([^;]*)\);" % name, gpu_h)
    assert m, "bloomgpu.h does not declare " + name
    return [re.split(r"[ *]", p.strip())[-1] for p in m.group(1).replace("\n", " ").split(",")]


def test_header_library_and_ctypes_agree():
    wide = declared("bsg_match_rows_wide")
    assert wide == ["ctx", "rows", "row_off", "n_rows", "cond_bytes", "cond_off", "cond_kinds", "n_conds", "prog_ops", "prog_off", "n_queries",
                    "set_first_row", "set_query_off", "set_queries", "n_sets", "tok", "out_bits", "out_fallback_rows", "fallback_cap", "out_n_fallback"]
    size = declared("bsg_match_wide_size")
    assert size == ["set_first_row", "set_query_off", "n_sets", "n_rows", "n_queries", "out_pair_word_off", "out_total_words"]
    assert "bsg_match_rows_wide" in _lib.EXPORTS and "bsg_match_wide_size" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.bsg_match_rows_wide.argtypes) == len(wide) and len(L.bsg_match_wide_size.argtypes) == len(size)
    n = C.c_uint32()
    assert L.bsg_match_rows_wide(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, 0,
                                 C.byref(n)) == _lib.BSG_E_INVALID


def wide_size(first, off, n_rows, n_queries, want_off=True):
    L = _lib.load()
    sfr = None if first is None else np.asarray(first, dtype=np.uint32)
    sqo = None if off is None else np.asarray(off, dtype=np.uint32)
    n_sets = 0 if sfr is None else len(sfr) - 1
    n_pairs = n_queries if sqo is None else int(sqo[-1])
    pwo = np.full(n_pairs + 1, 0xDEAD, dtype=np.uint64)
    total = C.c_uint64(0xDEAD)
    rc = L.bsg_match_wide_size(None if sfr is None else sfr.ctypes.data, None if sqo is None else sqo.ctypes.data, n_sets, n_rows, n_queries,
                               pwo.ctypes.data if want_off else None, C.byref(total))
    return rc, [int(x) for x in pwo], int(total.value)


def restated(first, off):
    pwo, at = [], 0
    for s in range(len(first) - 1):
        for _ in range(off[s], off[s + 1]):
            pwo.append(at)
            at += (first[s + 1] - first[s] + 63) // 64
    return pwo + [at], at


def test_wide_size_equals_the_restatement():
    sizes = [0, 1, 63, 64, 65, 10, 130]                                                # set sizes 0, 1, 63, 64, 65
    first = [0] + [int(x) for x in np.cumsum(sizes)]
    off = [0, 3, 4, 4, 6, 7, 7, 77]                                                    # sets 2 and 5 have no pair
    rc, pwo, total = wide_size(first, off, first[-1], 100)
    assert rc == _lib.BSG_OK and (pwo, total) == restated(first, off)
    assert total == 3 * 0 + 1 * 1 + 2 * 1 + 1 * 2 + 70 * 3
    rc, _, total2 = wide_size(first, off, first[-1], 100, want_off=False)
    assert rc == _lib.BSG_OK and total2 == total
    for n_rows, nq in ((0, 5), (1, 1), (63, 2), (64, 2), (65, 3), (1000, 300), (10, 0)):   # the implicit set: the planes of bsg_match_rows_many
        rc, pwo, total = wide_size(None, None, n_rows, nq)
        w = (n_rows + 63) // 64
        assert rc == _lib.BSG_OK and total == nq * w and pwo == [q * w for q in range(nq + 1)]


def test_wide_size_refuses_malformed_tables():
    L = _lib.load()
    first, off = [0, 10, 10, 100], [0, 2, 2, 5]
    assert wide_size(first, off, 100, 9)[0] == _lib.BSG_OK
    I = _lib.BSG_E_INVALID
    assert wide_size(first, off, 101, 9)[0] == I and wide_size([1, 10, 10, 100], off, 100, 9)[0] == I       # does not span [0, n_rows)
    assert wide_size([0, 10, 9, 100], off, 100, 9)[0] == I                                                 # set_first_row not monotone
    assert wide_size(first, [0, 2, 1, 5], 100, 9)[0] == I and wide_size(first, [1, 2, 2, 5], 100, 9)[0] == I   # set_query_off not monotone / not from 0
    sfr, sqo = np.asarray(first, dtype=np.uint32), np.asarray(off, dtype=np.uint32)
    total = C.c_uint64()
    assert L.bsg_match_wide_size(None, sqo.ctypes.data, 3, 100, 9, None, C.byref(total)) == I              # null arguments
    assert L.bsg_match_wide_size(sfr.ctypes.data, None, 3, 100, 9, None, C.byref(total)) == I
    assert L.bsg_match_wide_size(sfr.ctypes.data, sqo.ctypes.data, 3, 100, 9, None, None) == I
    assert L.bsg_match_wide_size(sfr.ctypes.data, sqo.ctypes.data, 0, 100, 9, None, C.byref(total)) == I   # a table without its number of sets
    msg = L.bsg_last_error(None)
    assert msg and b"set" in msg


def test_compiled_wide_batch_holds_300_queries():
    conds = [Q.FieldToken("f%d" % (i % 8), "t%d" % i) for i in range(40)] + [Q.Token("w%d" % i) for i in range(12)] + [Q.Field("p.%d" % i) for i in range(8)]
    rng = np.random.default_rng(2)
    exprs = []
    for q in range(300):
        kids = [conds[int(i)] for i in rng.choice(len(conds), size=int(rng.integers(1, 20)), replace=False)]
        exprs.append([Q.And(*kids), Q.Or(*kids), Q.And(kids[0], Q.Or(*kids[1:])), None, Q.And()][q % 5])
    exprs[7] = (Q.Token("w1"), Q.FieldRegex("f1", "^t"))                               # a (bloom, regex) pair, as CompiledRowQueryBatch takes them
    b = Q.CompiledWideBatch(exprs)
    assert b.n_queries == 300 and len(b.prog_off) == 301 and len(b.kinds) <= 64
    table = list(zip(b.kinds, b.fields, b.tokens))
    assert len(set(table)) == len(table) and (_lib.KIND_FIELD_REGEX, b"f1", b"^t") in table
    assert sum(Q.lowered_ops(b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]]) for q in range(300)) > 2048      # beyond the batched calls' LDS
    for q, e in enumerate(exprs):
        one = Q.CompiledRowQuery(*e) if isinstance(e, tuple) else Q.CompiledMatcher(e)
        prog = b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]]
        assert len(prog) == len(one.prog_ops)
        for got, want in zip(prog, one.prog_ops):
            assert got >> 28 == want >> 28
            if want >> 28 == _lib.OP_TERM:
                i, j = got & 0x0FFFFFFF, want & 0x0FFFFFFF
                assert table[i] == (one.kinds[j], one.fields[j], one.tokens[j]) and b.index_maps[q][j] == i
            else:
                assert got == want
    with pytest.raises(ValueError):
        Q.CompiledWideBatch([Q.Token("t%d" % i) for i in range(65)])                   # 65 distinct conditions still raise
    with pytest.raises(ValueError):
        Q.CompiledWideBatch([(None, Q.FieldRegex("f%d" % i, "x")) for i in range(17)])   # ... and 17 regex conditions
    with pytest.raises(ValueError):
        Q.CompiledMatcherBatch([Q.Token("t")] * 65)                                    # the batched compiler keeps its 64 queries
    assert Q.CompiledWideBatch([Q.Token("t")] * 65).n_queries == 65


def test_go_binding_has_the_wide_call():
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsWide(" in src and "C.bsg_match_rows_wide(" in src and "C.bsg_match_wide_size(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
