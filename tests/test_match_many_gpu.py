"""bsg_match_rows_many (k_match_rows_many): a batch of queries over one table of distinct conditions in one upload and one walk.
Every check compares with something that is not the code under test: the single-query call bsg_match_rows(_tok), the host
matcher Hst.match_row, or the tokenizer restatement."""
import ctypes as C

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q, synth
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import Context
from oracle import walker_oracle as W
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_collisions import pair
from tests.test_host_tables import KEYS, _random_value, go_marshal

pytestmark = pytest.mark.gpu

INVALID_UTF8 = b'{"s":"\xff\xfe bad utf8"}'
BAD_ROWS = [b'{"s":"\\xff\\xfe bad utf8 token"}', b'{"a": [1, 2', ('{' + '"a":{' * 17 + '"x":1' + '}' * 17 + '}').encode()]


def random_rows(rng, n):
    return [go_marshal({KEYS[rng.integers(0, len(KEYS))]: _random_value(rng, 0) for _ in range(rng.integers(1, 6))}) for _ in range(n)]


def expression_generator(rng, rows):
    vocab, paths = set(), set()
    for r in rows:
        f, t, _ = W.index_row(r)
        vocab |= t
        paths |= f
    vocab, paths = sorted(vocab), sorted(paths)

    def rand_expr(depth=0):
        r = rng.random()
        if depth >= 3 or r < 0.5:
            k = rng.integers(0, 3)
            tok = vocab[rng.integers(0, len(vocab))] if rng.random() < 0.85 else "absent%d" % rng.integers(0, 99)
            fld = paths[rng.integers(0, len(paths))] if rng.random() < 0.85 else "nope.%d" % rng.integers(0, 9)
            return [Q.Field(fld), Q.Token(tok), Q.FieldToken(fld, tok)][k]
        kids = [rand_expr(depth + 1) for _ in range(int(rng.integers(0, 4)))]
        return Q.And(*kids) if rng.random() < 0.5 else Q.Or(*kids)
    return rand_expr


def log_queries(n, base=0):
    """three-term And(FieldToken ...) over the synth rows' fields, the bench's query shape"""
    d = synth.draws(base, max(n, 1))
    return [Q.And(Q.FieldToken("level", synth.LEVELS[d["level"][i]]), Q.FieldToken("service", synth.SERVICES[d["service"][i]]),
                  Q.FieldToken("nested.region", "region-%d" % int(d["region"][i]))) for i in range(n)]


def singles(ctx, rows, exprs, tokenizer=None):
    out = [ctx.match_rows(rows, Q.CompiledMatcher(e), tokenizer) for e in exprs]
    union = sorted(set(int(r) for _, fb in out for r in fb))
    return np.array([h for h, _ in out], dtype=bool).reshape(len(exprs), len(rows)), union


def batch_that_fits(rng, gen, n, exprs):
    """exprs filled up to n with random expressions whose distinct conditions fit one table"""
    exprs = list(exprs)
    while len(exprs) < n:
        e = gen()
        try:
            Q.CompiledMatcherBatch(exprs + [e])
        except ValueError:
            e = exprs[int(rng.integers(0, len(exprs)))]          # the table is full: repeat a query (its conditions are in it)
        exprs.append(e)
    return exprs


@pytest.mark.parametrize("n_queries", [1, 2, 63, 64])
def test_many_call_equals_single_calls(ctx, n_queries):
    rng = np.random.default_rng(100 + n_queries)
    rows = synth.rows_json(3000, 600) + random_rows(rng, 500)
    gen = expression_generator(rng, rows[600:800])
    # query 0 has matches in both kinds of rows, whatever the generator draws
    exprs = [Q.Or(Q.FieldToken("level", "error"), Q.Field(KEYS[0]))] + log_queries(n_queries // 3, 3000)
    exprs = batch_that_fits(rng, gen, n_queries, exprs[:n_queries])
    batch = Q.CompiledMatcherBatch(exprs)
    planes, fb = ctx.match_rows_many(rows, batch)
    want, fb_union = singles(ctx, rows, exprs)
    assert planes.shape == (n_queries, len(rows))
    assert np.array_equal(planes, want)                                            # bit-identical planes
    assert [int(r) for r in fb] == fb_union                                        # exact: with all-ones masks every condition is live
    assert len(fb) < len(rows) / 4
    assert not planes[:, fb].any()
    for r in fb:                                                                   # the host matcher decides the rows handed back
        for q, e in enumerate(exprs):
            planes[q, r] = Hst.match_row(e, rows[int(r)])
    step = 1 if n_queries <= 2 else 7
    for q in range(n_queries):
        for r in range(q % step, len(rows), step):
            assert bool(planes[q, r]) == Hst.match_row(exprs[q], rows[r]), (q, r)
    assert planes.sum() > 50


def test_pure_log_rows_hand_nothing_back(ctx):
    """On synth rows the device decides everything itself: the comparison cannot be satisfied by handing rows to the host."""
    rows = synth.rows_json(0, 5000)
    d = synth.draws(0, 5000)
    exprs = log_queries(64)
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(exprs))
    assert len(fb) == 0 and ctx.last_match_ms() > 0
    dq = synth.draws(0, 64)
    for q in range(64):
        want = (d["level"] == dq["level"][q]) & (d["service"] == dq["service"][q]) & (d["region"] == dq["region"][q])
        assert np.array_equal(planes[q], want), q
    assert planes.sum() > 100
    want, fb_union = singles(ctx, rows, exprs[:5])
    assert fb_union == [] and np.array_equal(planes[:5], want)


def test_expression_edge_cases_inside_one_batch(ctx):
    # evalMatcherNode (row_matcher.go:257-290): nil => true, And() => true, Or() => false, unknown => false, nil condition => true
    rows = [b'{"a":"x"}', b'{"b":"y"}', b'{}', b'[1,2]']
    unknown_expr = {"ExpressionType": "XOR", "Children": []}
    unknown_cond = {"ExpressionType": "CONDITION", "Condition": {"Type": "BOGUS", "Field": "a", "Token": "x"}}
    nil_cond = {"ExpressionType": "CONDITION", "Condition": None}
    cases = [(None, [True] * 4), (Q.And(), [True] * 4), (Q.Or(), [False] * 4), (unknown_expr, [False] * 4),
             (unknown_cond, [False] * 4), (nil_cond, [True] * 4), (Q.Or(unknown_cond, Q.Field("a")), [True, False, False, False]),
             (Q.And(nil_cond, Q.Token("y")), [False, True, False, False]),
             (Q.And(Q.Or(Q.Field("a"), Q.Field("b")), Q.Or(Q.Token("x"), Q.And())), [True, True, False, False])]
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch([e for e, _ in cases]))
    assert len(fb) == 0
    for q, (e, want) in enumerate(cases):
        assert list(map(bool, planes[q])) == want, e
        assert [Hst.match_row(e, r) for r in rows] == want
    # FieldToken is the (path, token) pair at one leaf, never the joined key (row_matcher.go:587)
    rows = [b'{"a::b":"c"}', b'{"a":"b::c"}', b'{"a":"x","b":"y"}', b'{"a":["p","q"],"b":{"a":"q2"}}']
    cases = [(Q.FieldToken("a", "b::c"), [False, True, False, False]), (Q.FieldToken("a::b", "c"), [True, False, False, False]),
             (Q.FieldToken("a", "y"), [False, False, False, False]),
             (Q.FieldToken("a", "q"), [False, False, False, True]), (Q.FieldToken("b.a", "q2"), [False, False, False, True]),
             (Q.And(Q.FieldToken("a", "x"), Q.FieldToken("b", "y")), [False, False, True, False])]
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch([e for e, _ in cases]))
    assert len(fb) == 0
    for q, (e, want) in enumerate(cases):
        assert list(map(bool, planes[q])) == want, e
        assert [Hst.match_row(e, r) for r in rows] == want
    # targets are never normalised, rows are folded
    rows = [b'{"name":"ALICE Smith"}', '{"name":"Ünï ÀB ΩMEGA"}'.encode(), b'{"n":1E5,"t":true,"z":null}']
    cases = [(Q.Token("alice"), [True, False, False]), (Q.Token("ALICE"), [False, False, False]),
             (Q.Token("ünï"), [False, True, False]), (Q.Token("àb"), [False, True, False]), (Q.Token("ωmega"), [False, True, False]),
             (Q.FieldToken("n", "1e5"), [False, False, True]), (Q.FieldToken("n", "100000"), [False, False, False]),
             (Q.FieldToken("t", "true"), [False, False, True]), (Q.Field("z"), [False, False, True]),
             (Q.FieldToken("z", "null"), [False, False, False])]
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch([e for e, _ in cases]))
    assert len(fb) == 0
    for q, (e, want) in enumerate(cases):
        assert list(map(bool, planes[q])) == want, e


class RawBatch:
    """a batch whose condition strings are raw bytes (a collision partner is not text)"""

    def __init__(self, conds, programs):
        self.kinds = [k for k, _, _ in conds]
        self.fields = [f for _, f, _ in conds]
        self.tokens = [t for _, _, t in conds]
        self.prog_ops, self.prog_off = [], [0]
        for p in programs:
            self.prog_ops += p
            self.prog_off.append(len(self.prog_ops))


def test_sets_and_masks(ctx):
    rows = synth.rows_json(7000, 1000)
    exprs = log_queries(5, 7000) + [None, Q.Token("error"), Q.Field("nested.az")]
    nq = len(exprs)
    batch = Q.CompiledMatcherBatch(exprs)
    full, fb = ctx.match_rows_many(rows, batch)
    assert len(fb) == 0 and full[5].all() and full.sum() > 1200
    # sets of uneven sizes (one of them empty, cuts inside 64-row words), every kind of mask
    first = [0, 1, 64, 100, 100, 333, 640, 999, 1000]
    masks = [0b00000001, 0b11111111, 0, 0b10100000, 0b01010101, 0b00100000, 0b11011111, 0b10000000]
    planes, fb = ctx.match_rows_many(rows, batch, first, masks)
    assert len(fb) == 0
    for s, m in enumerate(masks):
        for q in range(nq):
            got = planes[q, first[s]: first[s + 1]]
            if (m >> q) & 1:
                assert np.array_equal(got, full[q, first[s]: first[s + 1]]), (s, q)
            else:
                assert not got.any(), (s, q)
    # one set with all-ones mask == no sets at all
    planes, fb = ctx.match_rows_many(rows, batch, [0, len(rows)], [(1 << nq) - 1])
    assert np.array_equal(planes, full) and len(fb) == 0
    # rows the device cannot decide: an invalid-UTF-8 row and a murmur collision with a table condition
    a, b = pair(3)
    rows = [b'{"k":"ok"}'] * 70 + [INVALID_UTF8, b'{"k":"' + a + b'"}'] + [b'{"k":"ok"}'] * 60
    raw = RawBatch([(_lib.KIND_TOKEN, b"", b), (_lib.KIND_TOKEN, b"", b"ok")], [[_lib.op(_lib.OP_TERM, 1)], [_lib.op(_lib.OP_TERM, 0)]])
    for cm, want_fb in ((RawBatch([(_lib.KIND_TOKEN, b"", b"ok")], [[0]]), [70]), (RawBatch([(_lib.KIND_TOKEN, b"", b)], [[0]]), [70, 71])):
        m = Q.CompiledMatcher(None)
        m.kinds, m.fields, m.tokens, m.prog_ops = cm.kinds, cm.fields, cm.tokens, cm.prog_ops
        assert [int(r) for r in ctx.match_rows(rows, m)[1]] == want_fb             # the single call agrees on what these rows are
    planes, fb = ctx.match_rows_many(rows, raw, [0, 70, 72, len(rows)], [0b11, 0, 0b01])
    assert len(fb) == 0                                                            # mask 0: never a fallback row, whatever its bytes
    assert planes[0, :70].all() and not planes[:, 70:72].any() and planes[0, 72:].all() and not planes[1].any()
    for m in (0b01, 0b10, 0b11):
        # a non-zero mask: both go to the host once - the collision is with a TABLE condition, whichever query owns it
        planes, fb = ctx.match_rows_many(rows, raw, [0, 70, 72, len(rows)], [0b11, m, 0b01])
        assert [int(r) for r in fb] == [70, 71] and not planes[:, 70:72].any()
    planes, fb = ctx.match_rows_many(rows, raw)
    assert [int(r) for r in fb] == [70, 71]


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257, 4100])
def test_shapes(ctx, n_rows):
    rows = synth.rows_json(11000, n_rows)
    if n_rows > 200:
        rows[n_rows - 1] = BAD_ROWS[1]
        rows[130] = BAD_ROWS[2]
    exprs = log_queries(9, 11000) + [None, Q.Or(Q.Token("warn"), Q.Token("error"))]
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(exprs))
    want, fb_union = singles(ctx, rows, exprs)
    assert np.array_equal(planes, want) and [int(r) for r in fb] == fb_union
    assert fb_union == ([130, n_rows - 1] if n_rows > 200 else [])


def test_chunk_cuts_and_device_counts(ctx):
    """Sets and 64-row words that straddle chunk cuts; every device count gives the single-device result."""
    rows = synth.rows_json(20000, 6000)
    where = [0, 255, 256, 257, 1023, 1024, 3000, 5998]
    for i, r in enumerate(where):
        rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
    exprs = log_queries(20, 20000) + [Q.Token("ok"), None]
    nq = len(exprs)
    batch = Q.CompiledMatcherBatch(exprs)
    rng = np.random.default_rng(9)
    first = [0] + sorted(int(x) for x in rng.integers(1, 6000, size=37)) + [6000]
    masks = [int(x) for x in rng.integers(0, 1 << nq, size=len(first) - 1)]
    masks[3] = 0
    masks[0] |= 1                                                                  # row 0 (a bad row) stays live
    live = np.zeros(6000, dtype=bool)
    for s, m in enumerate(masks):
        live[first[s]: first[s + 1]] = m != 0
    want_fb = [r for r in where if live[r]]
    want, _ = singles(ctx, rows, exprs)
    for s, m in enumerate(masks):
        for q in range(nq):
            if not (m >> q) & 1:
                want[q, first[s]: first[s + 1]] = False
    planes0, fb0 = ctx.match_rows_many(rows, batch, first, masks)
    assert np.array_equal(planes0, want) and [int(r) for r in fb0] == want_fb and len(want_fb) >= 2 and want.sum() > 100
    try:
        for chunk in (1 << 16, 70001, 1 << 18):                                    # (the library takes no chunk below 64 KiB)
            ctx.set_ingest_chunk(chunk)
            planes, fb = ctx.match_rows_many(rows, batch, first, masks)
            assert np.array_equal(planes, planes0) and np.array_equal(fb, fb0), chunk
    finally:
        ctx.set_ingest_chunk(0)
    for n_dev in (2, 3, 8):
        with Context(device_ids(n_dev)) as m:
            m.set_lab(7, 1)                                                        # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            planes, fb = m.match_rows_many(rows, batch, first, masks)
            assert np.array_equal(planes, planes0) and np.array_equal(fb, fb0), n_dev
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            m.set_ingest_chunk(1 << 16)
            planes, fb = m.match_rows_many(rows, batch)
            full, fb_full = ctx.match_rows_many(rows, batch)
            assert np.array_equal(planes, full) and np.array_equal(fb, fb_full) and [int(r) for r in fb] == where


@pytest.mark.parametrize("spec_name", ["punct_lower", "comma_semi"])
def test_separator_family_tokenizer(ctx, spec_name):
    spec = TR.SPECS[spec_name]
    rows = [b'{"msg":"user=alice,bob;Carol","path":"/var/log/app.log"}', b'{"msg":"alice bob","tags":["x,y","Z;w"]}',
            b'{"msg":"user=ALICE","n":1.5,"path":"a-b"}', b'{"other":"alice,carol"}'] * 40 + synth.rows_json(0, 100)
    exprs = [Q.Token("alice"), Q.Token("Carol"), Q.Token("carol"), Q.FieldToken("msg", "bob"), Q.FieldToken("tags", "y"), Q.Token("user=alice"),
             Q.And(Q.Token("alice"), Q.Or(Q.FieldToken("path", "log"), Q.FieldToken("other", "carol"))), Q.Token("alice bob"), None,
             Q.FieldToken("level", "error"), Q.Token("1.5"), Q.FieldToken("n", "5")]
    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(exprs), tokenizer=spec)
    want, fb_union = singles(ctx, rows, exprs, spec)
    assert np.array_equal(planes, want) and [int(r) for r in fb] == fb_union == []
    for q, e in enumerate(exprs):
        assert [bool(x) for x in planes[q]] == [TR.row_verdict(r, spec, e) for r in rows], (spec_name, q)
    default, _ = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(exprs))
    assert not np.array_equal(default, planes)                                     # the spec is not ignored
    masked, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(exprs), [0, 100, len(rows)], [0b101, 0b010], tokenizer=spec)
    assert np.array_equal(masked[0, :100], planes[0, :100]) and np.array_equal(masked[1, 100:], planes[1, 100:])
    assert not masked[0, 100:].any() and not masked[1, :100].any() and not masked[3:].any()


def raw_call(ctx, rows, batch, n_queries=None, set_first_row=None, masks=None, n_sets=None, prog_off=None):
    """the C call itself, with arguments the Python layer would refuse to build"""
    from bloomsearch_amd.gpu import pack_entries
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
    kinds = np.asarray(batch.kinds, dtype=np.uint32)
    ops = np.asarray(batch.prog_ops, dtype=np.uint32)
    poff = np.asarray(batch.prog_off if prog_off is None else prog_off, dtype=np.uint32)
    nq = len(poff) - 1 if n_queries is None else n_queries
    sfr = None if set_first_row is None else np.asarray(set_first_row, dtype=np.uint32)
    msk = None if masks is None else np.asarray(masks, dtype=np.uint64)
    ns = (0 if msk is None else len(msk)) if n_sets is None else n_sets
    bits = np.zeros((max(nq, 1), (len(rows) + 63) // 64), dtype=np.uint64)
    fb = np.zeros(len(rows), dtype=np.uint32)
    nfb = C.c_uint32()
    p = _lib._ptr
    return ctx.L.bsg_match_rows_many(ctx.h, p(blob), p(off), len(rows), p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq,
                                     p(sfr), p(msk), ns, None, p(bits), p(fb), len(fb), C.byref(nfb)), bits


def test_limits_and_malformed_arguments(ctx):
    rows = synth.rows_json(0, 130)
    good = Q.CompiledMatcherBatch(log_queries(3))
    before = ctx.device_calls()

    def refused(code, *a, **k):
        rc, bits = raw_call(ctx, rows, *a, **k)
        assert rc == code and not bits.any(), (rc, a, k)
        msg = ctx.L.bsg_last_error(ctx.h)
        assert msg and len(msg) > 10
        return msg.decode()

    U, I = _lib.BSG_E_UNSUPPORTED, _lib.BSG_E_INVALID
    assert "queries" in refused(U, RawBatch([(_lib.KIND_TOKEN, b"", b"t")], [[0]] * 65))                                     # 65 queries
    conds65 = [(_lib.KIND_TOKEN, b"", b"t%d" % i) for i in range(65)]
    assert "conditions" in refused(U, RawBatch(conds65, [[_lib.op(_lib.OP_TERM, i)] for i in range(3)]))                     # 65 conditions
    conds64 = conds65[:64]
    big = [_lib.op(_lib.OP_TERM, i) for i in range(64)] + [_lib.op(_lib.OP_AND, 64)]
    refused(U, RawBatch(conds64, [big] * 17))                                                                                # 17 x 127 lowered ops > 2 048
    deep = [_lib.op(_lib.OP_TERM, 0)] * 66 + [_lib.op(_lib.OP_OR, 2), _lib.op(_lib.OP_AND, 2)] * 32 + [_lib.op(_lib.OP_OR, 2)]
    refused(U, RawBatch(conds64, [[0], deep]))                                                                               # depth 66
    assert "FieldRegex" in refused(U, RawBatch([(_lib.KIND_FIELD_REGEX, b"level", b"err")], [[0]]))                          # a regex kind
    refused(I, RawBatch([(7, b"level", b"err")], [[0]]))                                                                     # an unknown kind
    refused(I, good, set_first_row=[1, 130], masks=[1])                                                                      # does not start at 0
    refused(I, good, set_first_row=[0, 129], masks=[1])                                                                      # does not end at n_rows
    refused(I, good, set_first_row=[0, 100, 50, 130], masks=[1, 1, 1])                                                       # not monotone
    refused(I, good, set_first_row=[0, 130], masks=[0b1000])                                                                 # bit 3 of 3 queries
    refused(I, good, n_sets=2)                                                                                               # sets announced, tables null
    refused(I, good, prog_off=[0, 5, 3, 15])                                                                                 # prog_off not monotone
    refused(I, RawBatch([(_lib.KIND_TOKEN, b"", b"t")], [[_lib.op(_lib.OP_TERM, 1)]]))                                       # a term outside the table
    with pytest.raises(BloomGpuError):
        ctx.match_rows_many(rows, RawBatch([(_lib.KIND_FIELD_REGEX, b"level", b"err")], [[0]]))
    assert np.array_equal(ctx.device_calls(), before)                                                                        # nothing was launched
    # empty calls are fine and write nothing
    rc, bits = raw_call(ctx, rows, good, n_queries=0)
    assert rc == 0 and not bits.any()
    assert ctx.match_rows_many([], good)[0].shape == (3, 0)
    assert np.array_equal(ctx.device_calls(), before)
    # the context is usable afterwards, and a batch exactly at the limits runs
    planes, fb = ctx.match_rows_many(rows, good)
    want, _ = singles(ctx, rows, log_queries(3))
    assert np.array_equal(planes, want) and len(fb) == 0
    rows2 = [b'{"m":"' + b" ".join(b"t%d" % i for i in range(k)) + b'"}' for k in (0, 1, 63, 64, 65)]
    at_cap = RawBatch(conds64, [big] * 16)
    planes, fb = ctx.match_rows_many(rows2, at_cap)
    assert len(fb) == 0 and [bool(x) for x in planes[15]] == [False, False, False, True, True]
