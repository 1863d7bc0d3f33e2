"""bsg_match_rows_wide (k_match_rows_store*, k_eval_row_programs): any number of queries over one condition table in one walk, the
result one bit row per listed (set, query) pair.  Every comparison is exact bit equality: each pair's row against the single call
(bsg_match_rows_tok of that program alone) restricted to the set, one small case against the oracle walker's matcher, and the
implicit set against bsg_match_rows_many's planes."""
import ctypes as C

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.gpu import Context, pack_entries, wide_pair_bits
from oracle import walker_oracle as W
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_collisions import pair as collision_pair
from tests.test_match_many_gpu import BAD_ROWS, RawBatch, log_queries

pytestmark = pytest.mark.gpu

DEEP_ROW = BAD_ROWS[2]                         # nesting depth 17: outside the device walker's envelope


def rx(field, pattern):
    return Q.FieldRegex(field, pattern)


def single(ctx, rows, item, tokenizer=None):
    m = Q.CompiledRowQuery(*item) if isinstance(item, tuple) else Q.CompiledMatcher(item)
    hits, fb = ctx.match_rows_regex(rows, m, tokenizer=tokenizer)
    return hits, set(int(r) for r in fb)


def csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return off, [q for l in lists for q in l]


def check_wide(ctx, rows, items, first=None, lists=None, tokenizer=None, batch=None, singles=None):
    """the wide call against the single calls; -> (per pair bool rows, fallback rows, singles)"""
    batch = batch or Q.CompiledWideBatch(items)
    nq = batch.n_queries
    if first is None:
        words, pwo, fb = ctx.match_rows_wide(rows, batch, tokenizer=tokenizer)
        first, lists = [0, len(rows)], [list(range(nq))]
    else:
        off, flat = csr(lists)
        words, pwo, fb = ctx.match_rows_wide(rows, batch, first, off, flat, tokenizer=tokenizer)
    fb = [int(r) for r in fb]
    assert fb == sorted(set(fb))
    singles = singles if singles is not None else {}
    out, p = [], 0
    for s, listed in enumerate(lists):
        lo, hi = first[s], first[s + 1]
        assert listed or not any(lo <= r < hi for r in fb)                             # rows of a set with no pair are never handed back
        assert listed == sorted(set(listed))
        in_fb = np.array([r in fb for r in range(lo, hi)], dtype=bool)
        for q in listed:
            if q not in singles:
                singles[q] = single(ctx, rows, items[q], tokenizer)
            hits, one_fb = singles[q]
            assert all(r in fb for r in one_fb if lo <= r < hi), (s, q)
            w = words[int(pwo[p]): int(pwo[p + 1])]
            assert len(w) == (hi - lo + 63) // 64
            bits = np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little").astype(bool)
            assert not bits[hi - lo:].any(), (s, q)                                    # bits past the set's last row are 0
            got = wide_pair_bits(words, pwo, p, hi - lo)
            assert np.array_equal(got, hits[lo:hi] & ~in_fb), (s, q)
            out.append(got)
            p += 1
    assert p == len(pwo) - 1 and int(pwo[-1]) == len(words)
    return out, fb, singles


def mixed_items(n, base=500):
    """n queries over at most 64 distinct conditions of the synth rows: three-term ANDs, ORs, constants, a few regex pairs"""
    logs = log_queries(40, base)
    extra = [Q.Token("error"), Q.Field("nested.az"), None, Q.And(), Q.Or(), Q.Or(Q.Token("warn"), Q.FieldToken("service", "auth")),
             (Q.FieldToken("level", "error"), rx("message", "timeout|cache")), (None, rx("service", "^pay")), (Q.Token("timeout"), rx("level", "^err"))]
    items = []
    for q in range(n):
        items.append(extra[q % len(extra)] if q % 4 == 3 else logs[(q * 7) % len(logs)])
        if q % 10 == 9:                                                                # wider programs: Or of ten three-term ANDs
            items[-1] = Q.Or(*[logs[(q + k) % len(logs)] for k in range(10)])
    return items


@pytest.mark.parametrize("n_queries", [1, 64, 65, 300])
def test_query_counts_equal_single_calls(ctx, n_queries):
    rows = synth.rows_json(500, 257)
    rows[100], rows[256] = DEEP_ROW, BAD_ROWS[0]
    items = mixed_items(n_queries)
    batch = Q.CompiledWideBatch(items)
    assert len(batch.kinds) <= 64
    if n_queries == 300:
        assert sum(Q.lowered_ops(batch.prog_ops[batch.prog_off[q]: batch.prog_off[q + 1]]) for q in range(300)) > 2048   # the old LDS limit
    out, fb, singles = check_wide(ctx, rows, items, batch=batch)
    assert fb == [100, 256] and sum(int(o.sum()) for o in out) > 0 and ctx.last_match_ms() > 0
    # sets: 1, 63, 64, 65 rows, a boundary inside a wave and inside a 256-row workgroup; queries listed sparsely, one set with none
    first = [0, 1, 64, 128, 193, 200, 257]
    rng = np.random.default_rng(n_queries)
    lists = [sorted(int(q) for q in rng.choice(n_queries, size=min(n_queries, int(rng.integers(1, 40))), replace=False)) for _ in range(6)]
    lists[4] = []
    out, fb, _ = check_wide(ctx, rows, items, first, lists, batch=batch, singles=singles)
    assert fb == [100, 256]


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_row_counts_and_the_plane_layout_of_the_batched_call(ctx, n_rows):
    rows = synth.rows_json(900, n_rows)
    exprs = log_queries(20, 900) + [None, Q.Token("error"), Q.Field("nested.az")]
    many = Q.CompiledMatcherBatch(exprs)
    planes, fb_many = ctx.match_rows_many(rows, many)
    words, pwo, fb = ctx.match_rows_wide(rows, Q.CompiledWideBatch(exprs))
    n_words = (n_rows + 63) // 64
    assert [int(x) for x in pwo] == [q * n_words for q in range(len(exprs) + 1)]
    got = np.unpackbits(words.view(np.uint8).reshape(len(exprs), n_words * 8), axis=1, bitorder="little").astype(bool)
    assert np.array_equal(got[:, :n_rows], planes) and not got[:, n_rows:].any() and len(fb) == 0 and len(fb_many) == 0
    assert planes[20].all()


def test_a_set_of_three_tiles_with_seventy_pairs_and_the_oracle(ctx):
    rows = synth.rows_json(2000, 130 + 20)
    items = mixed_items(70, 2000)[:61] + log_queries(9, 2100)                          # 70 queries, no regex pair among the last ones
    items = [e if not isinstance(e, tuple) else Q.Token("cache") for e in items]       # the oracle's matcher knows bloom expressions
    out, fb, _ = check_wide(ctx, rows, items, [0, 130, 150], [list(range(70)), [0, 69]])
    assert not fb and len(out) == 72
    for q in (0, 3, 9, 22, 69):                                                        # oracle/walker_oracle.py's matcher directly
        want = np.array([W.matches_bloom_expression(r, items[q]) if items[q] is not None else True for r in rows[:130]])
        assert np.array_equal(out[q], want), q


def test_sets_with_no_pair_are_not_walked(ctx):
    a, b = collision_pair(3)
    colliding = b'{"k":"' + a + b'"}'                                                  # emits a token with the hashes of condition b, not its bytes
    rows = synth.rows_json(0, 20) + [DEEP_ROW, colliding, BAD_ROWS[0]] + synth.rows_json(20, 20) + [DEEP_ROW, colliding, BAD_ROWS[0]] + synth.rows_json(40, 7)
    T = _lib.KIND_TOKEN
    term = lambda i: [_lib.op(_lib.OP_TERM, i)]
    batch = RawBatch([(T, b"", b"error"), (T, b"", b)], [term(0), term(1), []])
    first = [0, 23, 46, 53]
    off, flat = csr([[], [0, 2], [0]])
    before = ctx.device_calls().sum()
    words, pwo, fb = ctx.match_rows_wide(rows, batch, first, off, flat)
    assert [int(r) for r in fb] == [43, 44, 45]                                        # only where a query is listed; the collision counts
    assert ctx.device_calls().sum() == before + 1                                     # although no listed program references condition 1
    hits, _ = ctx.match_rows(rows, Q.CompiledMatcher(Q.Token("error")))
    assert np.array_equal(wide_pair_bits(words, pwo, 0, 23), hits[23:46] & (np.arange(23) < 20))
    assert np.array_equal(wide_pair_bits(words, pwo, 1, 23), np.arange(23) < 20)       # nil expression: every decided row; the handed-back rows' bits are 0
    assert np.array_equal(wide_pair_bits(words, pwo, 2, 7), hits[46:])
    # no pair at all: nothing is launched, nothing written
    words, pwo, fb = ctx.match_rows_wide(rows, batch, first, [0, 0, 0, 0], [])
    assert len(words) == 0 and len(fb) == 0 and ctx.device_calls().sum() == before + 2


def test_program_edge_cases_inside_one_call(ctx):
    rows = [b'{"a":"x"}', b'{"b":"y"}', b'{}', b'{"a":"x","b":"y","c":"z"}'] * 20
    nil_cond = {"ExpressionType": "CONDITION", "Condition": None}
    unknown = {"ExpressionType": "XOR", "Children": []}
    deep = Q.Token("x")
    for k in range(63):                                                                # a right-leaning chain: every level adds one to the depth, 64 in all
        deep = Q.And(Q.Field("a"), deep) if k % 2 else Q.Or(Q.Field("zz"), deep)
    wide_or = Q.Or(*[Q.Token("n%d" % i) for i in range(39)], Q.Token("z"))             # an n-ary Or of 40 terms
    cases = [(None, [1, 1, 1, 1]), (Q.And(), [1, 1, 1, 1]), (Q.Or(), [0, 0, 0, 0]), (nil_cond, [1, 1, 1, 1]), (unknown, [0, 0, 0, 0]),
             (wide_or, [0, 0, 0, 1]), (Q.And(Q.Or(Q.Field("a"), Q.Field("b")), Q.Or(Q.Token("x"), Q.And())), [1, 1, 0, 1]), (Q.Field("c"), [0, 0, 0, 1])]
    items = [e for e, _ in cases] + [deep]
    first = [0, 10, 40, 80]
    lists = [[0, 1, 2, 3, 4, 5, 6, 8], [0, 5, 8], [0, 2, 6]]                           # query 0 on every set, query 7 on none
    out, fb, _ = check_wide(ctx, rows, items, first, lists)
    assert not fb
    p = 0
    for s, listed in enumerate(lists):
        for q in listed:
            if q < len(cases):
                want = [bool(cases[q][1][r % 4]) for r in range(first[s], first[s + 1])]
                assert list(out[p]) == want, (s, q)
            p += 1
    # depth 65 is refused, before any launch
    deeper = Q.And(Q.Field("a"), deep)                                                 # deep's root is an Or: an And above it is one level more (an Or would be merged into it)
    before = ctx.device_calls().sum()
    with pytest.raises(_lib.BloomGpuError):
        ctx.match_rows_wide(rows, Q.CompiledWideBatch([deeper]))
    assert ctx.device_calls().sum() == before


def test_regex_conditions_are_opened_by_the_sets_condition_mask(ctx):
    pats = ["timeout|cache", "timeout|retry", "b.*a", "a", "x"]                        # five regex conditions on one field: a lane holds four
    items = [(None, rx("message", p)) for p in pats] + [(Q.FieldToken("level", "error"), rx("message", "a")), Q.FieldToken("service", "auth")]
    rows = synth.rows_json(100, 300)
    for r, text in ((5, b'{"level":"info"}'), (130, b'{"message":null}'), (250, b'{"msg":"timeout"}')):
        rows[r] = text
    first = [0, 100, 200, 300]
    out, fb, singles = check_wide(ctx, rows, items, first, [[0, 1, 2, 5, 6], [1, 2, 3, 4, 6], [0, 4]])
    assert not fb and sum(int(o.sum()) for o in out) > 50                              # at most four of the five per set: nothing handed back
    out, fb, _ = check_wide(ctx, rows, items, first, [[0, 1, 2, 5, 6], [0, 1, 2, 3, 4], [0, 4]], singles=singles)
    assert fb == [r for r in range(100, 200) if r != 130]                              # the set that uses all five: its rows with a message text
    spec = TR.SPECS["punct_lower"]                                                     # one separator-family tokenizer spec
    out, fb, _ = check_wide(ctx, rows, items, first, [[0, 5, 6], [], [3, 5, 6]], tokenizer=spec)
    assert not fb and sum(int(o.sum()) for o in out) > 20


def test_chunks_and_device_counts(ctx):
    rows = synth.rows_json(20000, 3000)
    where = [0, 255, 1023, 2998]
    for i, r in enumerate(where):
        rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
    items = mixed_items(90, 20000)
    batch = Q.CompiledWideBatch(items)
    rng = np.random.default_rng(11)
    first = [0] + sorted(int(x) for x in rng.integers(1, 3000, size=9)) + [3000]
    first[5] = first[4]                                                                # an empty set
    lists = [sorted(int(q) for q in rng.choice(90, size=int(rng.integers(1, 80)), replace=False)) for _ in range(10)]
    lists[2] = []
    off, flat = csr(lists)
    out0, fb0, _ = check_wide(ctx, rows, items, first, lists, batch=batch)
    words0, pwo0, _ = ctx.match_rows_wide(rows, batch, first, off, flat)
    assert len(fb0) >= 2 and sum(int(o.sum()) for o in out0) > 100
    try:
        ctx.set_ingest_chunk(1 << 16)                                                  # ~750 KB of rows: at least three chunks, sets cut by them
        words, pwo, fb = ctx.match_rows_wide(rows, batch, first, off, flat)
        assert words.tobytes() == words0.tobytes() and [int(r) for r in fb] == fb0
    finally:
        ctx.set_ingest_chunk(0)
    for n_dev in (2, 3):
        with Context(device_ids(n_dev)) as m:
            m.set_lab(7, 1)                                                            # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            words, pwo, fb = m.match_rows_wide(rows, batch, first, off, flat)
            assert words.tobytes() == words0.tobytes() and pwo.tobytes() == pwo0.tobytes() and [int(r) for r in fb] == fb0, n_dev
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            big = [0, 3000]                                                            # one set: every part boundary cuts it
            w1, p1, f1 = m.match_rows_wide(rows, batch, big, [0, 90], list(range(90)))
            w0, p0, f0 = ctx.match_rows_wide(rows, batch)
            assert w1.tobytes() == w0.tobytes() and p1.tobytes() == p0.tobytes() and f1.tobytes() == f0.tobytes() and [int(r) for r in f1] == where


def raw_wide(ctx, rows, batch, first=None, off=None, flat=None, n_queries=None):
    """the C call itself, with arguments the Python layer would refuse to build"""
    roff = np.zeros(len(rows) + 1, dtype=np.uint64)
    roff[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
    kinds = np.asarray(batch.kinds, dtype=np.uint32)
    ops = np.asarray(batch.prog_ops, dtype=np.uint32)
    poff = np.asarray(batch.prog_off, dtype=np.uint32)
    nq = len(poff) - 1 if n_queries is None else n_queries
    arr = lambda v: None if v is None else np.asarray(v, dtype=np.uint32)
    sfr, sqo, sq = arr(first), arr(off), arr(flat)
    bits = np.zeros(max(nq, 1) * ((len(rows) + 63) // 64) + 64, dtype=np.uint64)
    fb = np.zeros(len(rows), dtype=np.uint32)
    nfb = C.c_uint32()
    p = _lib._ptr
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = ctx.L.bsg_match_rows_wide(ctx.h, p(blob), p(roff), len(rows), p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq,
                                   ptr(sfr), ptr(sqo), ptr(sq), 0 if sfr is None else len(sfr) - 1, None, p(bits), p(fb), len(fb), C.byref(nfb))
    assert rc == _lib.BSG_OK or not bits.any()
    return rc


def test_limits_and_malformed_arguments(ctx):
    rows = synth.rows_json(0, 130)
    before = ctx.device_calls()
    U, I = _lib.BSG_E_UNSUPPORTED, _lib.BSG_E_INVALID
    term = lambda i: _lib.op(_lib.OP_TERM, i)
    R, T = _lib.KIND_FIELD_REGEX, _lib.KIND_TOKEN
    one = RawBatch([(T, b"", b"error")], [[term(0)], []])

    def message():
        return ctx.L.bsg_last_error(ctx.h).decode()

    assert raw_wide(ctx, rows, RawBatch([(T, b"", b"t%d" % i) for i in range(65)], [[term(0)]])) == U and "conditions" in message()
    assert raw_wide(ctx, rows, RawBatch([(R, b"f%d" % i, b"x") for i in range(17)], [[term(i)] for i in range(17)])) == U and "regex conditions" in message()
    assert raw_wide(ctx, rows, RawBatch([(R, b"a", b"\\bx")], [[term(0)]])) == U and "regex condition 0" in message()
    lens = [989 + i for i in range(12)]                                                # twelve ~1 000-state DFAs of ~4 250 bytes: over 46 592 bytes of tables
    assert raw_wide(ctx, rows, RawBatch([(R, b"f%d" % i, b"^[0-9a-f]{%d}$" % n) for i, n in enumerate(lens)], [[term(i)] for i in range(12)])) == U
    assert "LDS" in message()
    deep = [term(0)] * 66 + [_lib.op(_lib.OP_OR, 2), _lib.op(_lib.OP_AND, 2)] * 32 + [_lib.op(_lib.OP_OR, 2)]
    assert raw_wide(ctx, rows, RawBatch([(T, b"", b"t")], [[term(0)], deep])) == U and "deep" in message()
    too_many = Q.MATCH_WIDE_MAX_QUERIES + 1
    assert raw_wide(ctx, rows, RawBatch([(T, b"", b"t")], [[term(0)]]), n_queries=too_many) == U and "queries" in message()
    n_terms = Q.MATCH_WIDE_MAX_OPS // 2 + 1                                            # one flat Or of n terms lowers to 2 n - 1 ops at depth 2
    assert raw_wide(ctx, rows, RawBatch([(T, b"", b"t")], [[term(0)] * n_terms + [_lib.op(_lib.OP_OR, n_terms)]])) == U and "ops" in message()
    # malformed
    assert raw_wide(ctx, rows, one, [0, 130], [0, 2], None) == I                       # null set_queries
    assert raw_wide(ctx, rows, one, [0, 130], None, [0, 1]) == I and raw_wide(ctx, rows, one, None, [0, 2], [0, 1]) == I
    assert raw_wide(ctx, rows, one, [0, 129], [0, 2], [0, 1]) == I and raw_wide(ctx, rows, one, [1, 130], [0, 2], [0, 1]) == I
    assert raw_wide(ctx, rows, one, [0, 70, 60, 130], [0, 1, 1, 2], [0, 1]) == I       # set_first_row not monotone
    assert raw_wide(ctx, rows, one, [0, 60, 130], [0, 2, 1], [0, 1]) == I              # set_query_off not monotone
    assert raw_wide(ctx, rows, one, [0, 130], [0, 2], [1, 0]) == I and raw_wide(ctx, rows, one, [0, 130], [0, 2], [0, 0]) == I   # not strictly ascending
    assert raw_wide(ctx, rows, one, [0, 130], [0, 2], [0, 2]) == I and "query 2" in message()
    bad_off = RawBatch([(T, b"", b"error")], [[term(0)], []])
    bad_off.prog_off = [0, 1, 0]
    assert raw_wide(ctx, rows, bad_off) == I
    assert raw_wide(ctx, rows, RawBatch([(T, b"", b"error")], [[term(1)]])) == I       # a program that references condition 1 of 1
    assert np.array_equal(ctx.device_calls(), before)                                  # nothing was launched
    # the context still works; sixteen regex conditions and 64 conditions are within the call
    words, pwo, fb = ctx.match_rows_wide([b'{"f3":"x"}'], Q.CompiledWideBatch([(None, rx("f%d" % i, "x|y")) for i in range(16)]))
    assert [int(w) for w in words] == [int(i == 3) for i in range(16)] and not len(fb)
    assert raw_wide(ctx, rows, one, [0, 64, 130], [0, 2, 3], [0, 1, 1]) == _lib.BSG_OK
    # ten such tables (~42 500 bytes) are beyond the batched call's 38 140 bytes and within this one's
    tall = [('{"f9":"%s"}' % ("ab" * 500)[:lens[9]]).encode(), ('{"f9":"%s"}' % ("c" * (lens[9] - 1))).encode(), ('{"f0":"%s"}' % ("0" * lens[0])).encode()]
    ten = [(None, rx("f%d" % i, "^[0-9a-f]{%d}$" % lens[i])) for i in range(10)]
    words, pwo, fb = ctx.match_rows_wide(tall, Q.CompiledWideBatch(ten))
    assert [int(w) for w in words] == [4, 0, 0, 0, 0, 0, 0, 0, 0, 1] and not len(fb)
    with pytest.raises(_lib.BloomGpuError):
        ctx.match_rows_many_regex(tall, Q.CompiledRowQueryBatch(ten))
