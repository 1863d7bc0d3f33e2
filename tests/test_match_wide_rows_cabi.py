"""bsg_match_rows_wide_rows' surface without a GPU: the header declares it and bsg_match_pair_rows_list with the documented argument
names, the built library exports them, ctypes binds them with matching arity, a null context is refused before anything else,
bsg_match_pair_rows_list (host arithmetic, no context) expands every tag and refuses headers that are no pair of the set, the bound
of the payload follows from bsg_match_wide_size, and the Go binding agrees with the header."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bloomsearch_amd import _lib
from bloomsearch_amd.gpu import BloomGpuError, pair_rows_list
from tests.test_match_wide_cabi import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ALL, LIST, DENSE = range(4)


def test_header_library_and_ctypes_agree():
    rows = declared("bsg_match_rows_wide_rows")
    wide = declared("bsg_match_rows_wide")
    assert rows[:16] == wide[:16] and rows[15] == "tok"                                # the bit-row call's arguments up to and including tok
    assert rows[16:] == ["out_pair_hdr", "out_pair_off", "out_payload", "payload_cap", "out_payload_len", "out_fallback_rows", "fallback_cap", "out_n_fallback"]
    lst = declared("bsg_match_pair_rows_list")
    assert lst == ["hdr", "payload", "set_rows", "out_rows", "cap", "out_n"]
    assert "bsg_match_rows_wide_rows" in _lib.EXPORTS and "bsg_match_pair_rows_list" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.bsg_match_rows_wide_rows.argtypes) == len(rows) and len(L.bsg_match_pair_rows_list.argtypes) == len(lst)
    n, length = C.c_uint32(), C.c_uint64(7)
    assert L.bsg_match_rows_wide_rows(None, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, None, None, 0,
                                      C.byref(length), None, 0, C.byref(n)) == _lib.BSG_E_INVALID
    assert b"ctx" in L.bsg_last_error(None) and length.value == 7                      # refused before anything is written
    hdr = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert "#define BSG_MATCH_PAIR_SCAN_WIDTH" in hdr


def test_pair_rows_list_without_a_context():
    R = 150                                                                            # T = 3: a LIST holds at most 5 rows
    bits = np.zeros(192, dtype=np.uint8)
    bits[[0, 31, 32, 63, 64, 100, 149]] = 1
    dense = np.packbits(bits, bitorder="little").view("<u4")
    assert pair_rows_list(NONE << 30, [], R).tolist() == []
    assert pair_rows_list(ALL << 30, [], R).tolist() == list(range(R))
    assert pair_rows_list(LIST << 30 | 4, [0, 63, 64, 149], R).tolist() == [0, 63, 64, 149]
    assert pair_rows_list(DENSE << 30, dense, R).tolist() == [0, 31, 32, 63, 64, 100, 149]
    assert pair_rows_list(NONE << 30, [], 0).tolist() == []                            # a set without rows
    # *out_n is the full count whatever cap is; at most cap indices are written
    L = _lib.load()
    out = np.full(8, 0xFEED, dtype=np.uint32)
    n = C.c_uint32()
    assert L.bsg_match_pair_rows_list(DENSE << 30, dense.ctypes.data, R, out.ctypes.data, 3, C.byref(n)) == _lib.BSG_OK
    assert n.value == 7 and out.tolist() == [0, 31, 32] + [0xFEED] * 5
    assert L.bsg_match_pair_rows_list(ALL << 30, None, R, None, 0, C.byref(n)) == _lib.BSG_OK and n.value == R
    assert pair_rows_list(LIST << 30 | 4, [0, 63, 64, 149], R, cap=2).tolist() == [0, 63]
    I = _lib.BSG_E_INVALID
    assert L.bsg_match_pair_rows_list(LIST << 30 | 4, None, R, out.ctypes.data, 8, C.byref(n)) == I      # null arguments
    assert L.bsg_match_pair_rows_list(ALL << 30, None, R, None, 8, C.byref(n)) == I
    assert L.bsg_match_pair_rows_list(ALL << 30, None, R, out.ctypes.data, 8, None) == I
    for hdr, payload in ((LIST << 30 | 6, [0, 1, 2, 3, 4, 5]), (LIST << 30, []), (LIST << 30 | 3, [5, 4, 9]), (LIST << 30 | 2, [5, 150]),
                         (ALL << 30 | 150, []), (NONE << 30 | 1, []), (DENSE << 30 | 7, dense)):
        with pytest.raises(BloomGpuError) as e:
            pair_rows_list(hdr, payload, R)
        assert e.value.code == I and "150 rows" in str(e.value)
    past = dense.copy()
    past[4] |= 1 << 22                                                                 # row 150 of 150
    with pytest.raises(BloomGpuError):
        pair_rows_list(DENSE << 30, past, R)
    with pytest.raises(BloomGpuError):
        pair_rows_list(ALL << 30, [], 0)                                               # no set without rows is ALL


def test_the_bit_rows_bound_the_payload():
    """2 u32 per word of bsg_match_wide_size is the capacity that cannot be too small: no tag's payload exceeds its pair's bit row"""
    L = _lib.load()
    first = np.asarray([0, 0, 1, 64, 129, 258], dtype=np.uint32)
    off = np.asarray([0, 2, 3, 3, 10, 12], dtype=np.uint32)
    total = C.c_uint64()
    assert L.bsg_match_wide_size(first.ctypes.data, off.ctypes.data, 5, 258, 20, None, C.byref(total)) == _lib.BSG_OK
    longest = 0
    for s in range(5):
        R = int(first[s + 1] - first[s])
        T = (R + 63) // 64
        longest += int(off[s + 1] - off[s]) * max([2 * T if R > 2 * T else 0, min(2 * T - 1, max(R - 1, 0))])   # DENSE where it exists, else the longest LIST
    assert longest <= 2 * total.value and total.value == 0 * 2 + 1 + 0 + 2 * 7 + 3 * 2


def test_go_binding_has_the_rows_call():
    src = open(os.path.join(ROOT, "go", "bloomgpu", "bloomgpu.go")).read()
    assert "func (g *Context) MatchRowsWideRows(" in src and "C.bsg_match_rows_wide_rows(" in src and "C.bsg_match_pair_rows_list(" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
