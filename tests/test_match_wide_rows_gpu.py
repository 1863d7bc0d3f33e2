"""bsg_match_rows_wide_rows (k_pair_sizes, k_pair_scan_*, k_pair_write behind k_eval_row_programs): each listed (set, query) pair's
matches as a tagged row list.  The reference of every case is bsg_match_rows_wide on the same inputs, expanded on the host (that call
is held to the oracle walker by tests/test_match_wide_gpu.py; one case here goes to the oracle's matcher directly): decoded lists,
counts, tags, offsets and fallback rows are equal, a pair's tag is the contract's function of (c, R), and the result is
byte-identical for any number of devices and any chunk size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.gpu import Context, pack_entries, pair_rows_list, wide_pair_bits
from oracle import walker_oracle as W
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_match_many_gpu import BAD_ROWS, log_queries
from tests.test_match_wide_gpu import csr, mixed_items

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ALL, LIST, DENSE = range(4)
DEEP_ROW = BAD_ROWS[2]                         # nesting depth 17: outside the device walker's envelope


def tiles(n):
    return -(-n // 64)


def want_tag(c, R):
    return NONE if c == 0 else ALL if c == R else LIST if c < 2 * tiles(R) else DENSE


def check_rows(ctx, rows, batch, first=None, lists=None, tokenizer=None, ref_ctx=None):
    """the list call against the bit-row call on the same inputs -> (headers, offsets, payload, fallback rows, per pair its rows)"""
    nq = len(batch.prog_off) - 1
    if first is None:
        sets = (None, None, None)
        first, lists = [0, len(rows)], [list(range(nq))]
    else:
        off, flat = csr(lists)
        sets = (first, off, flat)
    words, pwo, fb_w = (ref_ctx or ctx).match_rows_wide(rows, batch, *sets, tokenizer=tokenizer)
    hdr, poff, payload, fb = ctx.match_rows_wide_rows(rows, batch, *sets, tokenizer=tokenizer)
    assert fb.tobytes() == fb_w.tobytes()
    assert len(hdr) == len(pwo) - 1 == len(poff) - 1 and int(poff[0]) == 0 and int(poff[-1]) == len(payload)
    assert len(payload) <= 2 * len(words)                                              # never more than the bit rows
    decoded, p = [], 0
    for s, listed in enumerate(lists):
        R = first[s + 1] - first[s]
        for _ in listed:
            want = np.flatnonzero(wide_pair_bits(words, pwo, p, R))
            tag, n = int(hdr[p]) >> 30, int(hdr[p]) & 0x3FFFFFFF
            assert tag == want_tag(len(want), R), (s, p, len(want), R)
            assert n == (len(want) if tag == LIST else 0)
            size = n if tag == LIST else 2 * tiles(R) if tag == DENSE else 0
            assert int(poff[p + 1]) - int(poff[p]) == size, (s, p)
            mine = payload[int(poff[p]): int(poff[p + 1])]
            if tag == DENSE:                                                           # exactly the words of the bit-row call
                assert mine.tobytes() == np.ascontiguousarray(words[int(pwo[p]): int(pwo[p + 1])]).tobytes()
            got = pair_rows_list(hdr[p], mine, R)
            assert got.tolist() == want.tolist(), (s, p)
            decoded.append(got)
            p += 1
    assert p == len(hdr)
    return hdr, poff, payload, [int(r) for r in fb], decoded


def token_rows(R, tokens_of):
    """R rows whose message holds the tokens tokens_of(i) (and one no query names)"""
    return [('{"m":"%s"}' % " ".join(["pad%d" % i] + tokens_of(i))).encode() for i in range(R)]


def spread(R, c):
    """c of R row indices, the first and the last row and both sides of a tile boundary among them where they fit"""
    keep = [i for i in (0, R - 1, 63, 64) if 0 <= i < R]
    rest = [i for i in range(R) if i not in keep]
    rng = np.random.default_rng(R * 131 + c)
    picked = sorted(set(keep))[:c]
    picked += [int(x) for x in rng.choice(rest, size=c - len(picked), replace=False)] if c > len(picked) else []
    return set(picked)


def test_every_tag_on_sets_around_the_tile_size(ctx):
    sizes = [1, 63, 64, 65, 129, 0, 40, 0]                                             # set 6 (40 rows) has no pair; sets 5 and 7 have pairs and no rows
    rows, first = [], [0]
    for R in sizes:
        T = tiles(R)
        lst, dns = spread(R, max(min(2 * T - 1, R), 0)), spread(R, min(2 * T, R))
        rows += token_rows(R, lambda i: ["all"] + (["lst"] if i in lst else []) + (["dns"] if i in dns else []))
        first.append(first[-1] + R)
    items = [Q.Token("never"), Q.Token("all"), Q.Token("lst"), Q.Token("dns"), None]   # NONE, ALL, LIST at 2T - 1, DENSE at 2T, and the nil program
    lists = [[0, 1, 2, 3, 4]] * 6 + [[]] + [[1, 4]]
    hdr, poff, payload, fb, decoded = check_rows(ctx, rows, Q.CompiledWideBatch(items), first, lists)
    assert not fb
    tags = [int(h) >> 30 for h in hdr]
    assert tags[0:5] == [NONE, ALL, ALL, ALL, ALL]                                     # one row: everything but NONE is ALL
    for s, R in ((1, 63), (2, 64), (3, 65), (4, 129)):
        assert tags[5 * s: 5 * s + 5] == [NONE, ALL, LIST, DENSE, ALL], R
        assert int(hdr[5 * s + 2]) & 0x3FFFFFFF == 2 * tiles(R) - 1 and len(decoded[5 * s + 3]) == 2 * tiles(R)
    assert tags[25:30] == [NONE] * 5 and tags[30:] == [NONE, NONE]                     # sets without rows, in the middle and at the end


def test_a_row_outside_the_envelope_keeps_a_full_set_from_all(ctx):
    rows = token_rows(65, lambda i: ["all"])
    rows[40] = DEEP_ROW
    hdr, poff, payload, fb, decoded = check_rows(ctx, rows, Q.CompiledWideBatch([Q.Token("all"), None]), [0, 65], [[0, 1]])
    assert fb == [40]
    for p in (0, 1):                                                                   # 64 of 65 rows: DENSE, the handed-back row's bit 0
        assert int(hdr[p]) >> 30 == DENSE and decoded[p].tolist() == [i for i in range(65) if i != 40]


def test_the_implicit_set_a_regex_condition_a_tokenizer_and_the_oracle(ctx):
    rows = synth.rows_json(500, 257)
    rows[100], rows[256] = DEEP_ROW, BAD_ROWS[0]
    items = mixed_items(70)
    assert any(isinstance(e, tuple) for e in items)                                    # (bloom, FieldRegex) pairs among them
    batch = Q.CompiledWideBatch(items)
    assert _lib.KIND_FIELD_REGEX in batch.kinds
    hdr, _, _, fb, _ = check_rows(ctx, rows, batch)                                    # NULL set tables: n_pairs = n_queries
    assert fb == [100, 256] and len(hdr) == 70 and {LIST, DENSE, NONE} <= {int(h) >> 30 for h in hdr}
    spec = TR.SPECS["punct_lower"]
    _, _, _, fb, decoded = check_rows(ctx, rows, batch, [0, 100, 200, 257], [[0, 3, 7, 11], [], list(range(70))], tokenizer=spec)
    assert 100 not in fb and sum(len(d) for d in decoded) > 50                          # row 100 lies in the set without a pair
    # oracle/walker_oracle.py's matcher directly
    plain = [e for e in items if not isinstance(e, tuple) and e is not None][:12]
    good = synth.rows_json(2000, 130)
    _, _, _, fb, decoded = check_rows(ctx, good, Q.CompiledWideBatch(plain), [0, 130], [list(range(len(plain)))])
    assert not fb
    for q, e in enumerate(plain):
        assert decoded[q].tolist() == [i for i, r in enumerate(good) if W.matches_bloom_expression(r, e)], q


def scan_width():
    hdr = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    return int(re.search(r"#define BSG_MATCH_PAIR_SCAN_WIDTH (\d+)u", hdr).group(1))


def test_three_thousand_pairs_span_several_scan_workgroups(ctx):
    W_ = scan_width()
    n_sets = 10
    n_queries = max(300, (3 * W_ + n_sets) // n_sets + 1)
    while (n_queries * n_sets) % W_ == 0:
        n_queries += 1
    n_pairs = n_queries * n_sets
    assert n_pairs >= 3000 and n_pairs > 3 * W_ and n_pairs % W_ != 0                  # three full workgroups of the scan and a partial one
    rows = synth.rows_json(9000, 700)
    items = mixed_items(n_queries, 9000)
    first = list(range(0, 701, 70))
    hdr, poff, payload, fb, _ = check_rows(ctx, rows, Q.CompiledWideBatch(items), first, [list(range(n_queries))] * n_sets)
    assert len(hdr) == n_pairs and not fb and {NONE, ALL, LIST, DENSE} <= {int(h) >> 30 for h in hdr}
    assert int(poff[W_]) > 0 and int(poff[-1]) > int(poff[3 * W_]) > int(poff[2 * W_]) > int(poff[W_])     # payload behind every workgroup's base


def test_chunks_and_device_counts_give_the_same_bytes(ctx):
    rows = synth.rows_json(20000, 1000)
    rows[300], rows[700] = DEEP_ROW, BAD_ROWS[0]
    items = mixed_items(40, 20000) + [None, Q.Token("error"), Q.FieldToken("level", "error"), Q.Token("never-there")]
    batch = Q.CompiledWideBatch(items)
    nq = len(items)
    first = [0, 200, 400, 800, 800, 1000]                                              # a 200-row and a 400-row set, an empty one
    lists = [list(range(0, nq, 3)), list(range(nq)), list(range(nq)), [0, 40], list(range(1, nq, 2))]
    off, flat = csr(lists)
    # where equal bytes cut the call for 2 and 3 devices: inside the 400-row set, and inside the 200-row set and the 400-row one
    ends = np.cumsum([len(r) for r in rows])
    cut = lambda num, den: int(np.searchsorted(ends, ends[-1] * num // den))
    assert 400 + 64 < cut(1, 2) < 800 and 200 + 64 < cut(1, 3) < 400 and 400 + 64 < cut(2, 3) < 800
    hdr0, poff0, payload0, fb0, _ = check_rows(ctx, rows, batch, first, lists)
    assert fb0 == [300, 700]
    cut_sets = [int(h) >> 30 for h in hdr0[off[1]: off[3]]]
    assert {NONE, ALL, LIST, DENSE} <= set(cut_sets) | {int(h) >> 30 for h in hdr0}
    same = lambda got: (got[0].tobytes(), got[1].tobytes(), got[2].tobytes(), got[3].tobytes()) == (hdr0.tobytes(), poff0.tobytes(), payload0.tobytes(),
                                                                                                    np.asarray(fb0, dtype=np.uint32).tobytes())
    try:
        ctx.set_ingest_chunk(1)                                                        # the smallest chunk (64 KiB): ~250 KB of rows, sets span chunks
        assert same(ctx.match_rows_wide_rows(rows, batch, first, off, flat))
    finally:
        ctx.set_ingest_chunk(0)
    for n_dev in (1, 2, 3):
        with Context(device_ids(n_dev)) as m:
            m.set_lab(7, 1)                                                            # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            assert same(m.match_rows_wide_rows(rows, batch, first, off, flat)), n_dev
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            if n_dev == 3:
                check_rows(m, rows, batch, first, lists, ref_ctx=ctx)                  # ... and the stitched pairs decode to the bit rows


def raw_rows(ctx, rows, batch, cap, sentinel=0xA5A5A5A5):
    """the C call itself with a payload buffer of `cap` u32 (and room behind it), prefilled -> (rc, hdr, off, payload buffer, len)"""
    roff = np.zeros(len(rows) + 1, dtype=np.uint64)
    roff[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
    kinds = np.asarray(batch.kinds, dtype=np.uint32)
    ops = np.asarray(batch.prog_ops, dtype=np.uint32)
    poff = np.asarray(batch.prog_off, dtype=np.uint32)
    nq = len(poff) - 1
    hdr = np.full(nq, 0xFFFFFFFF, dtype=np.uint32)
    off = np.full(nq + 1, 0xFFFFFFFF, dtype=np.uint64)
    payload = np.full(cap + 8, sentinel, dtype=np.uint32)
    length = C.c_uint64(0xDEAD)
    fb = np.zeros(len(rows), dtype=np.uint32)
    nfb = C.c_uint32()
    p = _lib._ptr
    rc = ctx.L.bsg_match_rows_wide_rows(ctx.h, p(blob), p(roff), len(rows), p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq,
                                        None, None, None, 0, None, hdr.ctypes.data, off.ctypes.data, payload.ctypes.data if cap else None, cap,
                                        C.byref(length), p(fb), len(fb), C.byref(nfb))
    return rc, hdr, off, payload, int(length.value)


def test_the_payload_capacity(ctx):
    rows = synth.rows_json(500, 200)
    items = log_queries(6, 500) + [Q.Token("error"), None, Q.Token("never-there")]
    batch = Q.CompiledWideBatch(items)
    hdr0, poff0, payload0, _ = ctx.match_rows_wide_rows(rows, batch)
    need = len(payload0)
    assert need > 8 and {LIST, DENSE} <= {int(h) >> 30 for h in hdr0}
    rc, hdr, off, payload, length = raw_rows(ctx, rows, batch, need)                   # exactly the needed length
    assert rc == _lib.BSG_OK and length == need and hdr.tobytes() == hdr0.tobytes() and off.tobytes() == poff0.tobytes()
    assert payload[:need].tobytes() == payload0.tobytes() and (payload[need:] == 0xA5A5A5A5).all()
    rc, hdr, off, payload, length = raw_rows(ctx, rows, batch, need - 1)               # one short
    assert rc == _lib.BSG_E_INVALID and length == need and hdr.tobytes() == hdr0.tobytes() and off.tobytes() == poff0.tobytes()
    assert (payload == 0xA5A5A5A5).all()                                               # no payload is written
    msg = ctx.L.bsg_last_error(ctx.h).decode()
    assert str(need) in msg and str(need - 1) in msg
    none = Q.CompiledWideBatch([Q.Token("never-there"), Q.Or()])                       # an all-NONE result needs no payload buffer at all
    rc, hdr, off, payload, length = raw_rows(ctx, rows, none, 0)
    assert rc == _lib.BSG_OK and length == 0 and hdr.tolist() == [0, 0] and off.tolist() == [0, 0, 0] and (payload == 0xA5A5A5A5).all()
    rc, hdr, off, _, length = raw_rows(ctx, [], none, 0)                               # no rows: every header NONE
    assert rc == _lib.BSG_OK and length == 0 and hdr.tolist() == [0, 0] and off.tolist() == [0, 0, 0]


def test_the_calls_own_arguments_are_checked_before_any_launch(ctx):
    from tests.test_match_many_gpu import RawBatch
    rows = synth.rows_json(0, 130)
    T = _lib.KIND_TOKEN
    term = lambda i: [_lib.op(_lib.OP_TERM, i)]
    one = RawBatch([(T, b"", b"error")], [term(0), []])
    roff = np.zeros(len(rows) + 1, dtype=np.uint64)
    roff[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)

    def call(batch, hdr=True, payload=True, length=True, cap=1000, first=None, off=None, flat=None):
        cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
        kinds, ops, poff = (np.asarray(a, dtype=np.uint32) for a in (batch.kinds, batch.prog_ops, batch.prog_off))
        arr = lambda v: None if v is None else np.asarray(v, dtype=np.uint32)
        sfr, sqo, sq = arr(first), arr(off), arr(flat)
        h, o, pl = np.zeros(16, dtype=np.uint32), np.zeros(17, dtype=np.uint64), np.zeros(1000, dtype=np.uint32)
        n, nfb, fb = C.c_uint64(), C.c_uint32(), np.zeros(len(rows), dtype=np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data
        return ctx.L.bsg_match_rows_wide_rows(ctx.h, blob.ctypes.data, roff.ctypes.data, len(rows), ptr(cblob), coff.ctypes.data, kinds.ctypes.data, len(kinds),
                                              ptr(ops), poff.ctypes.data, len(poff) - 1, ptr(sfr), ptr(sqo), ptr(sq), 0 if sfr is None else len(sfr) - 1, None,
                                              h.ctypes.data if hdr else None, o.ctypes.data, pl.ctypes.data if payload else None, cap,
                                              C.byref(n) if length else None, fb.ctypes.data, len(fb), C.byref(nfb))

    before = ctx.device_calls()
    I, U = _lib.BSG_E_INVALID, _lib.BSG_E_UNSUPPORTED
    assert call(one, length=False) == I and call(one, payload=False) == I and call(one, hdr=False) == I        # null outputs
    assert call(one, first=[0, 129], off=[0, 2], flat=[0, 1]) == I and call(one, first=[0, 130], off=[0, 2], flat=[1, 0]) == I   # the wide call's set checks
    assert call(RawBatch([(T, b"", b"t%d" % i) for i in range(65)], [term(0)])) == U                           # ... and its limits
    assert call(RawBatch([(_lib.KIND_FIELD_REGEX, b"a", b"\\bx")], [term(0)])) == U
    assert np.array_equal(ctx.device_calls(), before)                                                          # nothing was launched
    assert call(one, payload=False, cap=0) == I                                                                # the payload does not fit 0: reported after the run
    assert "0" in ctx.L.bsg_last_error(ctx.h).decode() and call(one) == _lib.BSG_OK
