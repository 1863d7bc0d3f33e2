"""bsg_match_rows_lookup / bsg_match_rows_lookup_rows (k_match_rows_lookup*, k_eval_row_programs_w): the wide row matcher over tables of
up to 1 024 Field / Token / FieldToken conditions, every emission resolved by hash lookup, ceil(n_conds / 64) flag words per row.
Expected verdicts come from the oracle walker's matcher (oracle/walker_oracle.py), never from the library; where a table fits the
shipped wide call, the two calls are compared word for word, header for header and fallback list for fallback list."""
import ctypes as C

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.gpu import Context, pack_entries, pair_rows_list, wide_pair_bits
from oracle import walker_oracle as W
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_collisions import pair as collision_pair
from tests.test_match_many_gpu import BAD_ROWS, RawBatch, log_queries

pytestmark = pytest.mark.gpu

DEEP_ROW = BAD_ROWS[2]                         # nesting depth 17: outside the device walker's envelope


def csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return off, [q for l in lists for q in l]


def oracle_bits(rows, expr):
    return np.array([True if expr is None else bool(W.matches_bloom_expression(r, expr)) for r in rows], dtype=bool)


def lookup_pairs(ctx, rows, batch, first=None, lists=None, tokenizer=None):
    """both calls -> (per pair bool row from the bits, fallback rows); the lists must expand to the same rows"""
    if first is None:
        sets, args = [(0, len(rows))] * batch.n_queries, ()
    else:
        off, flat = csr(lists)
        sets, args = [(first[s], first[s + 1]) for s, l in enumerate(lists) for _ in l], (first, off, flat)
    words, pwo, fb = ctx.match_rows_lookup(rows, batch, *args, tokenizer=tokenizer)
    hdr, poff, payload, fb_rows = ctx.match_rows_lookup_rows(rows, batch, *args, tokenizer=tokenizer)
    assert len(pwo) - 1 == len(sets) == len(hdr) and fb.tobytes() == fb_rows.tobytes()
    out = []
    for p, (lo, hi) in enumerate(sets):
        bits = wide_pair_bits(words, pwo, p, hi - lo)
        listed = pair_rows_list(int(hdr[p]), payload[int(poff[p]): int(poff[p + 1])], hi - lo)
        assert np.array_equal(np.flatnonzero(bits), listed), p
        out.append(bits)
    return out, [int(r) for r in fb]


@pytest.mark.parametrize("kind", ["token", "field_token"])
def test_identity_at_the_limit(ctx, kind):
    n = 1024
    if kind == "token":
        exprs = [Q.Token("t%d" % i) for i in range(n)]
        rows = [b'{"k":"t%d"}' % i for i in range(n)]
    else:
        exprs = [Q.FieldToken("f%d" % i, "t%d" % i) for i in range(n)]
        rows = [b'{"f%d":"t%d"}' % (i, i) for i in range(n)]
    batch = Q.CompiledLookupBatch(exprs)
    assert len(batch.kinds) == n and batch.n_queries == n
    before = ctx.device_calls().sum()
    words, pwo, fb = ctx.match_rows_lookup(rows, batch)
    assert ctx.device_calls().sum() == before + 1 and len(fb) == 0 and ctx.last_match_ms() > 0
    got = np.unpackbits(words.view(np.uint8).reshape(n, n // 8), axis=1, bitorder="little").astype(bool)
    assert np.array_equal(got, np.eye(n, dtype=bool))                                  # pair i matches exactly row i
    hdr, poff, payload, fb = ctx.match_rows_lookup_rows(rows, batch)
    assert len(fb) == 0 and all(int(h) == (2 << 30 | 1) for h in hdr)            # BSG_ROW_LIST, one row
    assert [int(x) for x in payload] == list(range(n)) and [int(x) for x in poff] == list(range(n + 1))
    for q in (0, 63, 64, 511, 1023):                                                   # the oracle's matcher on a few queries
        sample = [0, 1, 63, 64, 65, 510, 511, 512, 1022, 1023]
        assert np.array_equal(got[q][sample], oracle_bits([rows[r] for r in sample], exprs[q])), q


BOUNDARY = [63, 64, 127, 128]


def boundary_case(n_conds):
    terms = [Q.Token("t%d" % i) for i in range(n_conds)]
    at = [c for c in BOUNDARY if c < n_conds]
    exprs = list(terms)                                                                # query c = condition c alone: the table's order is the queries'
    for i, a in enumerate(at):
        for b in at[i + 1:]:
            exprs += [Q.And(terms[a], terms[b]), Q.Or(terms[a], terms[b])]
    exprs += [Q.And(*[terms[c] for c in at]), Q.Or(*[terms[c] for c in at]), Q.And(terms[0], Q.Or(terms[at[-1]], terms[n_conds - 1]))]
    return at, exprs


def boundary_rows(at, n_conds, n_rows):
    rows = []
    for r in range(n_rows):                                                            # every subset of the boundary conditions, and two others
        toks = ["t%d" % c for k, c in enumerate(at) if (r >> k) & 1] + ["t%d" % ((r * 7) % n_conds), "t0" if r % 3 == 0 else "zz"]
        rows.append(('{"m":"%s"}' % " ".join(toks)).encode())
    return rows


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_conds", [65, 128, 129])
def test_word_boundaries(ctx, n_conds, n_rows):
    at, exprs = boundary_case(n_conds)
    rows = boundary_rows(at, n_conds, n_rows)
    batch = Q.CompiledLookupBatch(exprs)
    assert len(batch.kinds) == n_conds
    out, fb = lookup_pairs(ctx, rows, batch)
    assert not fb
    for q in at + list(range(n_conds, len(exprs))):
        assert np.array_equal(out[q], oracle_bits(rows, exprs[q])), q
    assert out[at[0]].any() or n_rows == 1


def test_role_separation(ctx):
    conds = [Q.Field("a"), Q.Token("a"), Q.FieldToken("a", "x"), Q.FieldToken("a", "y"), Q.FieldToken("b", "x")]
    rows = [b'{"a":"x"}', b'{"b":"a"}', b'{"b":"y"}', b'{"c":"x y"}', b'{"a":{"d":"x"}}', b'{"a":"x::y"}']
    batch = Q.CompiledLookupBatch(conds)
    assert len(batch.kinds) == 5
    out, fb = lookup_pairs(ctx, rows, batch)
    assert not fb
    for q, e in enumerate(conds):                                                      # each condition on its own
        assert np.array_equal(out[q], oracle_bits(rows, e)), q
    assert list(out[1]) == [False, True, False, False, False, False]                   # "a" as a token: only where it is a word
    assert not out[0][1]                                                               # ... and as a path never where it is only a word
    assert list(out[2]) == [True, False, False, False, False, False]                   # the pair at ONE leaf: not "a.d", not the joined key
    assert not out[3].any() and not out[4].any()                                       # y under b, x under c: the halves of a pair on different leaves


def small_table_items(n):
    logs = log_queries(40, 500)
    extra = [Q.Token("error"), Q.Field("nested.az"), None, Q.And(), Q.Or(), Q.Or(Q.Token("warn"), Q.FieldToken("service", "auth")),
             Q.And(Q.Field("level"), Q.Token("timeout"))]
    return [extra[q % len(extra)] if q % 4 == 3 else logs[(q * 7) % len(logs)] for q in range(n)]


@pytest.mark.parametrize("tokenizer", [None, "punct_lower"])
def test_agreement_with_the_wide_call(ctx, tokenizer):
    spec = None if tokenizer is None else TR.SPECS[tokenizer]
    a, b = collision_pair(3)
    rows = synth.rows_json(500, 257)
    rows[100], rows[130], rows[256] = DEEP_ROW, b'{"k":"' + a + b'"}', BAD_ROWS[0]
    items = small_table_items(80)
    batch = Q.CompiledWideBatch(items)
    T = _lib.KIND_TOKEN
    batch.kinds.append(T), batch.fields.append(b""), batch.tokens.append(b)            # a condition no program references: its collision still counts
    assert len(batch.kinds) <= 64
    first = [0, 0, 1, 64, 128, 193, 200, 257]                                          # sets of 0, 1, 63, 64, 65, 7 and 57 rows
    rng = np.random.default_rng(5)
    lists = [sorted(int(q) for q in rng.choice(80, size=int(rng.integers(1, 40)), replace=False)) for _ in range(7)]
    lists[5] = []                                                                      # a set without pairs
    off, flat = csr(lists)
    for args in ((), (first, off, flat)):
        w0, p0, f0 = ctx.match_rows_wide(rows, batch, *args, tokenizer=spec)
        w1, p1, f1 = ctx.match_rows_lookup(rows, batch, *args, tokenizer=spec)
        assert w0.tobytes() == w1.tobytes() and p0.tobytes() == p1.tobytes() and f0.tobytes() == f1.tobytes()
        r0 = ctx.match_rows_wide_rows(rows, batch, *args, tokenizer=spec)
        r1 = ctx.match_rows_lookup_rows(rows, batch, *args, tokenizer=spec)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r0, r1))
        assert w0.any() and len(f0) >= 2
    if tokenizer is None:
        assert [int(r) for r in f0] == [100, 130, 256]


def test_chunks_and_parts(ctx):
    rows = synth.rows_json(7000, 1500)
    where = [0, 63, 64, 1499]
    for i, r in enumerate(where):
        rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
    assert sum(len(r) for r in rows) >= 3 * (1 << 16)                                  # at least three launches at the smallest chunk
    d = synth.draws(7000, 1500)
    exprs = [Q.FieldToken("user_id", str(int(u))) for u in sorted(set(int(x) for x in d["user_id"]))[:150]]
    exprs += log_queries(30, 7000) + [Q.Token("error"), Q.Field("nested.az"), None]
    batch = Q.CompiledLookupBatch(exprs)
    assert len(batch.kinds) > 128
    nq = batch.n_queries
    first = [0, 700, 700, 1500]
    lists = [list(range(nq)), list(range(nq)), list(range(0, nq, 3))]
    off, flat = csr(lists)
    w0, p0, f0 = ctx.match_rows_lookup(rows, batch, first, off, flat)
    r0 = ctx.match_rows_lookup_rows(rows, batch, first, off, flat)
    assert [int(r) for r in f0] == where and w0.any()
    bits = wide_pair_bits(w0, p0, nq - 3, 700)                                         # Token("error") on the first set, by the oracle
    want = oracle_bits([b'{}' if r in where else rows[r] for r in range(700)], exprs[nq - 3])   # the oracle reads no malformed row
    assert want.any() and np.array_equal(bits, want)
    try:
        ctx.set_ingest_chunk(1 << 16)
        w1, p1, f1 = ctx.match_rows_lookup(rows, batch, first, off, flat)
        r1 = ctx.match_rows_lookup_rows(rows, batch, first, off, flat)
    finally:
        ctx.set_ingest_chunk(0)
    assert w1.tobytes() == w0.tobytes() and f1.tobytes() == f0.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(r0, r1))
    with Context(device_ids(2)) as m:                                                  # two aliases of one device
        m.set_lab(7, 1)                                                                # every call is cut over the devices, however small
        m.set_lab(8, 1)
        before = m.device_calls()
        w2, p2, f2 = m.match_rows_lookup(rows, batch, first, off, flat)
        assert ((m.device_calls() - before) > 0).sum() == 2
        r2 = m.match_rows_lookup_rows(rows, batch, first, off, flat)
    assert w2.tobytes() == w0.tobytes() and p2.tobytes() == p0.tobytes() and f2.tobytes() == f0.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r0, r2))


def test_fallback_rows(ctx):
    a, b = collision_pair(3)
    colliding = b'{"k":"' + a + b'"}'                                                  # emits a token with the hashes of condition b, not its bytes
    good = [b'{"k":"t%d"}' % i for i in range(20)]
    rows = good + [DEEP_ROW, colliding] + good + [DEEP_ROW, colliding]
    T = _lib.KIND_TOKEN
    term = lambda i: [_lib.op(_lib.OP_TERM, i)]
    conds = [(T, b"", b"t%d" % i) for i in range(99)] + [(T, b"", b)]                  # condition 99: the collision partner, in the table's second word
    batch = RawBatch(conds, [term(3), term(99), []])
    first = [0, 22, 44]
    off, flat = csr([[0, 1, 2], []])
    words, pwo, fb = ctx.match_rows_lookup(rows, batch, first, off, flat)
    assert [int(r) for r in fb] == [20, 21]                                            # handed back where listed, not in the set without pairs
    assert list(np.flatnonzero(wide_pair_bits(words, pwo, 0, 22))) == [3]
    assert not wide_pair_bits(words, pwo, 1, 22).any()
    assert np.array_equal(wide_pair_bits(words, pwo, 2, 22), np.arange(22) < 20)       # nil expression: every decided row; the handed-back rows' bits are 0
    words, pwo, fb = ctx.match_rows_lookup(rows, batch)
    assert [int(r) for r in fb] == [20, 21, 42, 43]
    # both members of the pair in one table, in either order: a row that holds either is handed back, wherever the two strings were
    # placed in the probe run, exactly as by the wide call
    two = [b'{"k":"' + a + b'"}', b'{"k":"' + b + b'"}', b'{"k":"t1"}']
    for conds in ([(T, b"", a), (T, b"", b), (T, b"", b"t1")], [(T, b"", b), (T, b"", a), (T, b"", b"t1")]):
        both = RawBatch(conds, [term(0), term(1), term(2)])
        w1, _, f1 = ctx.match_rows_lookup(two, both)
        w0, _, f0 = ctx.match_rows_wide(two, both)
        assert [int(r) for r in f1] == [0, 1] and f1.tobytes() == f0.tobytes() and w1.tobytes() == w0.tobytes() and [int(x) for x in w1] == [0, 0, 4]


def raw_lookup(ctx, rows, batch, rows_call=False):
    roff = np.zeros(len(rows) + 1, dtype=np.uint64)
    roff[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
    kinds = np.asarray(batch.kinds, dtype=np.uint32)
    ops = np.asarray(batch.prog_ops, dtype=np.uint32)
    poff = np.asarray(batch.prog_off, dtype=np.uint32)
    nq = len(poff) - 1
    total = nq * ((len(rows) + 63) // 64)
    bits = np.zeros(2 * total + 64, dtype=np.uint64)
    fb = np.zeros(len(rows), dtype=np.uint32)
    nfb, length = C.c_uint32(), C.c_uint64()
    p = _lib._ptr
    head = (ctx.h, p(blob), p(roff), len(rows), p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq, None, None, None, 0, None)
    if rows_call:
        hdr = np.zeros(nq, dtype=np.uint32)
        rc = ctx.L.bsg_match_rows_lookup_rows(*head, p(hdr), None, p(bits), 2 * total, C.byref(length), p(fb), len(fb), C.byref(nfb))
    else:
        rc = ctx.L.bsg_match_rows_lookup(*head, p(bits), p(fb), len(fb), C.byref(nfb))
    assert rc == _lib.BSG_OK or not bits.any()
    return rc


@pytest.mark.parametrize("rows_call", [False, True])
def test_refusals(ctx, rows_call):
    rows = synth.rows_json(0, 70)
    U = _lib.BSG_E_UNSUPPORTED
    term = lambda i: _lib.op(_lib.OP_TERM, i)
    R, T = _lib.KIND_FIELD_REGEX, _lib.KIND_TOKEN
    message = lambda: ctx.L.bsg_last_error(ctx.h).decode()
    deep = Q.Token("x")
    for k in range(63):                                                                # a right-leaning chain of alternating And / Or: depth 64
        deep = Q.And(Q.Field("a"), deep) if k % 2 else Q.Or(Q.Field("zz"), deep)
    refused = [(RawBatch([(T, b"", b"t%d" % i) for i in range(1025)], [[term(0)]]), ("1025 conditions", "1024")),
               (RawBatch([(T, b"", b"t"), (R, b"service", b"^a")], [[term(0)]]), ("condition 1", "FieldRegex")),
               (Q.CompiledLookupBatch([Q.Token("x"), Q.And(Q.Field("a"), deep)]), ("query 1", "depth 65"))]   # one level more than deep
    for batch, words in refused:
        before = ctx.device_calls()
        assert raw_lookup(ctx, rows, batch, rows_call) == U
        assert all(w in message() for w in words), message()
        assert np.array_equal(ctx.device_calls(), before), words                       # refused before any launch
    # at the limits the call runs
    before = ctx.device_calls().sum()
    assert raw_lookup(ctx, rows[:3], Q.CompiledLookupBatch([deep]), rows_call) == _lib.BSG_OK
    assert raw_lookup(ctx, rows, RawBatch([(T, b"", b"t%d" % i) for i in range(1024)], [[term(1023)]]), rows_call) == _lib.BSG_OK
    assert ctx.device_calls().sum() == before + 2
