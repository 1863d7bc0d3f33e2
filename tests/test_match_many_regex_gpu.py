"""bsg_match_rows_many_regex (k_match_rows_many_regex): a batch of queries with FieldRegex conditions over one table in one upload
and one walk.  Two independent answers, as tests/test_match_regex_gpu.py: the oracle walker's candidate texts with the PY
restatements of the patterns (bloom side: the host matcher), and the single-query calls bsg_match_rows_regex / bsg_match_rows_tok.
Rows the batched call hands back are decided by the host matcher and the host DFA runner (bsh_regex_match) and compared too."""
import ctypes as C
import re

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q, synth
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import Context, pack_entries
from tests import tokenizer_restatement as TR
from oracle import walker_oracle as W
from tests.helpers import device_ids
from tests.test_host_tables import go_marshal
from tests.test_match_many_gpu import BAD_ROWS, RawBatch, log_queries
from tests.test_match_regex_gpu import PY, dfa_runner, leaves, random_rows

pytestmark = pytest.mark.gpu

SLOTS = 4                                     # regex conditions one leaf may feed at once in the batched kernels (bloomgpu.h)
MANY_CAP, SINGLE_CAP = 38140, 44544

# regex conditions over the synth rows' fields, patterns from PY; at most 3 meet on one leaf (message), 13 distinct
POOL = [("message", "timeout|cache"), ("message", "timeout|retry"), ("message", "b.*a"), ("level", "^err"), ("level", "(?i)error"),
        ("service", "^pay"), ("service", "a"), ("nested.region", "region-[37]$"), ("nested", "a"), ("tags", "timeout|cache"),
        ("user_id", "^[0-9]+$"), ("user_id", "^2$"), ("timestamp", "^-?[0-9]+(\\.[0-9]+)?$")]


def covers(a, path):
    return a != "" and (path == a or path.startswith(a + "."))


def co_active_bound(batch):
    fields = [f.decode() for k, f in zip(batch.kinds, batch.fields) if k == _lib.KIND_FIELD_REGEX]
    return max((sum(covers(a, f) for a in fields) for f in fields), default=0)


def regex_verdict(lv, regex, runner):
    """compileRegexExpression's rules (row_matcher.go:440-480) over a row's (path, candidate text) leaves"""
    if regex is None:
        return True
    et = regex.get("ExpressionType")
    if et == "CONDITION":
        c = regex.get("Condition")
        if c is None:
            return True
        f = c.get("Field", "")
        return f != "" and any(covers(f, p) and runner(c["Pattern"], t) for p, t in lv)
    kids = regex.get("Children") or []
    if et == "OR":
        return any(regex_verdict(lv, k, runner) for k in kids)
    if et == "AND":
        return all(regex_verdict(lv, k, runner) for k in kids)
    return False


def cached(runner):
    memo = {}

    def run(pattern, text):
        key = (pattern, text)
        if key not in memo:
            memo[key] = runner(pattern, text)
        return memo[key]
    return run


def py_cached():
    return cached(lambda pattern, text: re.search(PY[pattern], text) is not None)


def singles(ctx, rows, pairs, tokenizer=None):
    out = [ctx.match_rows_regex(rows, Q.CompiledRowQuery(b, r), tokenizer=tokenizer) for b, r in pairs]
    return np.array([h for h, _ in out], dtype=bool).reshape(len(pairs), len(rows)), [set(int(x) for x in fb) for _, fb in out]


def live_mask(n_queries, n_rows, first, masks):
    live = np.ones((n_queries, n_rows), dtype=bool)
    if first is not None:
        for s, m in enumerate(masks):
            for q in range(n_queries):
                live[q, first[s]: first[s + 1]] = (m >> q) & 1
    return live


def check_batch(ctx, rows, pairs, first=None, masks=None, tokenizer=None, oracle_step=1, runner=None):
    """the batched call against the single calls and the oracle; -> (planes with the handed-back rows decided, fallback rows)"""
    batch = Q.CompiledRowQueryBatch(pairs)
    planes, fb = ctx.match_rows_many_regex(rows, batch, first, masks, tokenizer=tokenizer)
    fb = [int(r) for r in fb]
    nq = len(pairs)
    assert planes.shape == (nq, len(rows)) and fb == sorted(set(fb))
    assert not planes[:, fb].any()                                                 # all plane bits of a row handed back are 0
    live = live_mask(nq, len(rows), first, masks)
    one, one_fb = singles(ctx, rows, pairs, tokenizer)
    decided = np.ones(len(rows), dtype=bool)
    decided[fb] = False
    for q in range(nq):
        assert np.array_equal(planes[q, decided], (one[q] & live[q])[decided]), (q, pairs[q])
    union = sorted(set(r for q in range(nq) for r in one_fb[q] if live[q, r]))
    assert set(fb) >= set(union)
    if co_active_bound(batch) <= SLOTS:
        assert fb == union
    # the rows handed back: the host matcher and the host DFA runner, per query live on the row's set
    dfa = cached(dfa_runner)
    lv = {}
    for r in fb:
        try:
            lv[r] = leaves(rows[r])
        except Exception:
            continue                                                               # not JSON: no query matches it, its bits stay 0
        for q, (bloom, regex) in enumerate(pairs):
            if live[q, r]:
                planes[q, r] = (bloom is None or Hst.match_row(bloom, rows[r], tokenizer)) and regex_verdict(lv[r], regex, dfa)
    # the oracle: the walker's leaves with the PY restatements; the bloom side by the oracle's set matcher under the default tokenizer,
    # by the host matcher under a spec (the oracle walker knows the default tokenizer only)
    def bloom_ok(bloom, row):
        if bloom is None:
            return True
        return W.matches_bloom_expression(row, bloom) if tokenizer is None else Hst.match_row(bloom, row, tokenizer)
    runner = runner or py_cached()
    for r in range(0, len(rows), 1):
        try:
            row_leaves = lv[r] if r in lv else leaves(rows[r])
        except Exception:
            assert r in fb or not live[:, r].any(), rows[r]                        # a row the oracle cannot parse is never decided on the device
            continue
        for q in range(r % oracle_step, nq, oracle_step):
            bloom, regex = pairs[q]
            want = bool(live[q, r]) and bloom_ok(bloom, rows[r]) and regex_verdict(row_leaves, regex, runner)
            assert bool(planes[q, r]) == want, (q, r, pairs[q], rows[r])
    return planes, fb


def rx(field, pattern):
    return Q.FieldRegex(field, pattern)


def mixed_queries(rng, n):
    """plain, regex-only and bloom AND regex queries over the synth rows' fields; regex conditions from POOL"""
    plain = log_queries(max(n, 4), 500) + [Q.Token("error"), Q.Field("nested.az"), None, Q.Or(Q.Token("warn"), Q.FieldToken("service", "auth"))]
    out = []
    for q in range(n):
        bloom = plain[int(rng.integers(0, len(plain)))] if rng.random() < 0.6 else None
        kind = q % 3
        if kind == 0:
            regex = None
        elif kind == 1:
            regex = rx(*POOL[int(rng.integers(0, len(POOL)))])
        else:
            kids = [rx(*POOL[int(rng.integers(0, len(POOL)))]) for _ in range(int(rng.integers(2, 4)))]
            regex = Q.RegexAnd(*kids) if rng.random() < 0.4 else Q.RegexOr(*kids)
        out.append((bloom, regex))
    return out


def test_reference_regex_tables_in_one_batch(ctx):
    # query_test.go:28-30, tokenizer_test.go:193-212, row_matcher_test.go:118-133 / :342 - the tables of tests/test_match_regex_gpu.py
    rows = [b'{"level":"error","message":"upstream timeout","service":"auth"}', b'{"level":"info","message":"timeout","service":"auth"}',
            b'{"level":"info","message":"ok","service":"payments"}', b'{"level":"error","message":"ok","service":"auth"}',
            b'{"users":[{"id":1,"name":"John","active":true},{"id":2,"name":"Jane","active":false}]}',
            b'{"users":[{"id":3,"name":"Alice","active":false}]}',
            go_marshal({"user": {"name": "alice", "id": 7}, "a": "x", "latency": 12.5, "tags": ["Beta gamma", "x::y"]}),
            go_marshal({"user": "bob", "a": {"b": "y"}, "latency": 3, "tags": []})]
    pairs = [(None, Q.RegexOr(Q.RegexAnd(rx("message", "timeout|retry"), rx("level", "^err")), rx("service", "^pay"))),
             (None, Q.RegexAnd(rx("users.name", "(?i)^jo"), Q.RegexOr(rx("users.active", "^true$"), rx("users.id", "^2$")))),
             (Q.Field("user.name"), rx("user.name", ".")), (Q.Token("alice"), rx("user", "\\Azzz-never-matches\\z")),
             (None, rx("user", "^[0-9]+$")), (None, rx("a", ".")), (None, rx("latency", "^-?[0-9]+(\\.[0-9]+)?$")), (None, rx("tags", "Beta")),
             (None, rx("", ".*")), (None, rx("no.such.path", ".*")), (None, Q.RegexOr()), (None, Q.RegexAnd()),
             (Q.Field("user"), {"ExpressionType": "CONDITION", "Condition": None})]
    planes, fb = check_batch(ctx, rows, pairs)
    assert not fb
    want = {0: [1, 0, 1, 0, 0, 0, 0, 0], 1: [0, 0, 0, 0, 1, 0, 0, 0], 2: [0] * 6 + [1, 0], 3: [0] * 8, 4: [0] * 6 + [1, 0], 5: [0] * 6 + [1, 1],
            6: [0] * 6 + [1, 1], 7: [0] * 6 + [1, 0], 8: [0] * 8, 9: [0] * 8, 10: [0] * 8, 11: [1] * 8, 12: [0] * 6 + [1, 1]}
    for q, w in want.items():
        assert [int(x) for x in planes[q]] == w, q


@pytest.mark.parametrize("n_queries", [2, 17, 64])
@pytest.mark.parametrize("spec_name", [None, "punct_lower"])
def test_mixed_batches_equal_single_calls_and_the_oracle(ctx, n_queries, spec_name):
    spec = None if spec_name is None else TR.SPECS[spec_name]
    rng = np.random.default_rng(300 + n_queries)
    n_synth = 640
    rows = synth.rows_json(500, n_synth) + random_rows(n_queries, 60) + [BAD_ROWS[1], BAD_ROWS[2]]
    pairs = mixed_queries(rng, n_queries)
    batch = Q.CompiledRowQueryBatch(pairs)
    assert co_active_bound(batch) <= SLOTS and (n_queries < 17 or batch.kinds.count(_lib.KIND_FIELD_REGEX) >= 10)
    step = 1 if n_queries <= 17 else 5
    planes, fb = check_batch(ctx, rows, pairs, tokenizer=spec, oracle_step=step)
    assert all(r >= n_synth for r in fb) and len(rows) - 2 in fb                   # the synth rows are decided on the device, all of them
    assert planes.sum() > 50
    # sets and masks: a set with mask 0 in the middle, set boundaries inside 64-row words, an empty set
    nq = n_queries
    all_q = (1 << nq) - 1
    first = [0, 70, 100, 100, 333, 640, 700, len(rows)]
    masks = [all_q, 0b01, all_q, 0, all_q & 0x5555555555555555, 0, all_q]
    masked, fb_masked = check_batch(ctx, rows, pairs, first, masks, tokenizer=spec, oracle_step=step)
    assert all(r >= 700 for r in fb_masked) and fb_masked == [r for r in fb if r >= 700]   # rows of a set with mask 0 are never handed back
    assert not masked[:, 100:333].any() and not masked[:, 640:700].any()
    assert np.array_equal(masked[:, :70], planes[:, :70]) and np.array_equal(masked[0, 70:100], planes[0, 70:100])


def test_synth_rows_hand_nothing_back(ctx):
    """On synth rows with co_active_bound within the slots the device decides everything: no check can pass by handing rows back."""
    rows = synth.rows_json(0, 3000)
    d = synth.draws(0, 3000)
    pairs = [(Q.FieldToken("level", "error"), Q.RegexOr(rx("message", "timeout|cache"), rx("nested.region", "region-[37]$"))),
             (None, rx("service", "^pay")), (Q.FieldToken("level", "error"), None), (None, rx("level", "^err")),
             (None, Q.RegexAnd(rx("message", "timeout|cache"), rx("message", "timeout|retry"), rx("message", "b.*a"), rx("nested", "a")))]
    batch = Q.CompiledRowQueryBatch(pairs)
    planes, fb = ctx.match_rows_many_regex(rows, batch)
    assert len(fb) == 0 and ctx.last_match_ms() > 0
    is_error = d["level"] == synth.LEVELS.index("error")
    assert np.array_equal(planes[1], d["service"] == synth.SERVICES.index("payment"))
    assert np.array_equal(planes[2], is_error) and np.array_equal(planes[3], is_error)
    words = [set(synth.WORDS[w] for w in d["words"][i]) for i in range(len(rows))]
    want0 = np.array([bool(is_error[i]) and (bool(words[i] & {"timeout", "cache"}) or d["region"][i] in (3, 7)) for i in range(len(rows))])
    assert np.array_equal(planes[0], want0) and want0.sum() > 100
    one, one_fb = singles(ctx, rows, pairs)
    assert np.array_equal(planes, one) and not any(one_fb)


def test_chunked_upload_and_device_counts(ctx):
    rows = synth.rows_json(20000, 6000)
    where = [0, 255, 256, 1023, 3000, 5998]
    for i, r in enumerate(where):
        rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
    rng = np.random.default_rng(11)
    pairs = mixed_queries(rng, 20)
    nq = len(pairs)
    batch = Q.CompiledRowQueryBatch(pairs)
    assert batch.kinds.count(_lib.KIND_FIELD_REGEX) >= 8
    first = [0] + sorted(int(x) for x in rng.integers(1, 6000, size=29)) + [6000]
    masks = [int(x) for x in rng.integers(0, 1 << nq, size=len(first) - 1)]
    masks[3] = 0
    masks[0] |= 1
    live = live_mask(nq, 6000, first, masks)
    one, one_fb = singles(ctx, rows, pairs)
    want = one & live
    want[:, where] = False
    want_fb = [r for r in where if live[:, r].any()]
    planes0, fb0 = ctx.match_rows_many_regex(rows, batch, first, masks)
    assert np.array_equal(planes0, want) and [int(r) for r in fb0] == want_fb and len(want_fb) >= 2 and want.sum() > 100
    try:
        for chunk in (1 << 16, 70001, 1 << 18):                                    # several chunks: the rows are ~1.5 MB
            ctx.set_ingest_chunk(chunk)
            planes, fb = ctx.match_rows_many_regex(rows, batch, first, masks)
            assert np.array_equal(planes, planes0) and np.array_equal(fb, fb0), chunk
    finally:
        ctx.set_ingest_chunk(0)
    for n_dev in (2, 8):
        with Context(device_ids(n_dev)) as m:
            m.set_lab(7, 1)                                                        # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            planes, fb = m.match_rows_many_regex(rows, batch, first, masks)
            assert np.array_equal(planes, planes0) and np.array_equal(fb, fb0), n_dev
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            m.set_ingest_chunk(1 << 16)
            planes, fb = m.match_rows_many_regex(rows, batch)
            full, fb_full = ctx.match_rows_many_regex(rows, batch)
            assert np.array_equal(planes, full) and np.array_equal(fb, fb_full) and [int(r) for r in fb] == where


def test_user_masks_open_a_condition_only_where_a_query_uses_it(ctx):
    """Six distinct regex conditions on `message`: a lane holds four.  A row is handed back only when the queries LIVE on its set
    put more than four on its message leaf."""
    n_cond = 6 if SLOTS == 4 else 10
    pats = ["timeout|cache", "timeout|retry", "b.*a", "a", "x", "Beta", "^err", "^pay", "region-[37]$", "^true$"][:n_cond]
    pairs = [(None, rx("message", p)) for p in pats]
    rows = synth.rows_json(100, 200)
    no_text = [b'{"level":"info"}', b'{"message":null}', b'{"message":{},"x":1}', b'{"msg":"timeout"}']
    for i, r in enumerate((5, 77, 130, 199)):
        rows[r] = no_text[i]
    half = n_cond // 2
    lo, hi = (1 << half) - 1, ((1 << half) - 1) << half
    planes, fb = check_batch(ctx, rows, pairs, [0, 100, 200], [lo, hi])
    assert not fb                                                                  # three (five) live conditions per leaf: nothing handed back
    assert planes[:half, :100].any() and planes[half:, 100:].any() and not planes[half:, :100].any() and not planes[:half, 100:].any()
    # the second set evaluates all of them: exactly its rows with a message text come back
    planes, fb = check_batch(ctx, rows, pairs, [0, 100, 200], [lo, lo | hi])
    assert fb == [r for r in range(100, 200) if r not in (130, 199)]
    # ... and the single call agrees on what such a row is when ONE query holds all the conditions
    _, fb_one = ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, Q.RegexOr(*[rx("message", p) for p in pats])))
    assert [int(r) for r in fb_one] == [r for r in range(200) if r not in (5, 77, 130, 199)]
    # a condition nobody's program references is never opened (its user mask is 0)
    unused = RawBatch([(_lib.KIND_FIELD_REGEX, b"message", p.encode()) for p in pats], [[_lib.op(_lib.OP_TERM, i)] for i in range(SLOTS)])
    planes, fb = ctx.match_rows_many_regex(rows, unused)
    assert len(fb) == 0 and planes.any()


def test_a_table_without_regex_conditions_is_the_plain_batched_call(ctx):
    rows = synth.rows_json(7000, 1000)
    rows[130], rows[999] = BAD_ROWS[2], BAD_ROWS[1]
    batch = Q.CompiledMatcherBatch(log_queries(9, 7000) + [None, Q.Token("error"), Q.Field("nested.az")])
    first, masks = [0, 1, 64, 100, 100, 333, 640, 999, 1000], [1, 0xFFF, 0, 0b10100000, 0b01010101, 0b00100000, 0xFDF, 0x800]
    for spec in (None, TR.SPECS["punct_lower"]):
        for sets in ((None, None), (first, masks)):
            a, fa = ctx.match_rows_many(rows, batch, *sets, tokenizer=spec)
            b, fb = ctx.match_rows_many_regex(rows, batch, *sets, tokenizer=spec)
            assert a.tobytes() == b.tobytes() and fa.tobytes() == fb.tobytes()
    assert a.any() and [int(r) for r in fa] == [130, 999]


def raw_call(fn, ctx, rows, batch):
    """the C call itself, with arguments the Python layer would refuse to build"""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    cblob, coff = pack_entries([s for p in zip(batch.fields, batch.tokens) for s in p])
    kinds = np.asarray(batch.kinds, dtype=np.uint32)
    ops = np.asarray(batch.prog_ops, dtype=np.uint32)
    poff = np.asarray(batch.prog_off, dtype=np.uint32)
    nq = len(poff) - 1
    bits = np.zeros((max(nq, 1), (len(rows) + 63) // 64), dtype=np.uint64)
    fb = np.zeros(len(rows), dtype=np.uint32)
    nfb = C.c_uint32()
    p = _lib._ptr
    return fn(ctx.h, p(blob), p(off), len(rows), p(cblob), p(coff), p(kinds), len(kinds), p(ops), poff.ctypes.data, nq, None, None, 0, None,
              p(bits), p(fb), len(fb), C.byref(nfb)), bits


def test_limits(ctx):
    rows = synth.rows_json(0, 130)
    before = ctx.device_calls()
    U = _lib.BSG_E_UNSUPPORTED

    def refused(batch, fn=None):
        rc, bits = raw_call(fn or ctx.L.bsg_match_rows_many_regex, ctx, rows, batch)
        assert rc == U and not bits.any(), rc
        msg = ctx.L.bsg_last_error(ctx.h)
        assert msg and len(msg) > 10
        return msg.decode()

    term = lambda i: _lib.op(_lib.OP_TERM, i)
    R, T = _lib.KIND_FIELD_REGEX, _lib.KIND_TOKEN
    assert "regex conditions" in refused(RawBatch([(R, b"f%d" % i, b"x") for i in range(17)], [[term(i)] for i in range(17)]))     # 17 regex conditions
    for pat in (b"\\pL", b"(a|b)*a(a|b){24}", b"(?m)^x", b"\\bx"):                                                                # outside the subset
        msg = refused(RawBatch([(T, b"", b"t"), (R, b"a", b"x"), (R, b"a", pat)], [[term(0)], [term(1), term(2), _lib.op(_lib.OP_OR, 2)]]))
        assert "regex condition 2" in msg, msg
    # a table between the two caps (nine ~1 000-state DFAs; its size by the estimate: tests/test_regex_groups.py): the single call takes it
    # in one program, the batched call refuses it
    lens = [991 + i for i in range(9)]
    conds = [(R, b"f%d" % i, b"^[0-9a-f]{%d}$" % n) for i, n in enumerate(lens)]
    assert "LDS" in refused(RawBatch(conds, [[term(i)] for i in range(9)]))
    assert "LDS" in refused(RawBatch(conds, [[term(i) for i in range(9)] + [_lib.op(_lib.OP_OR, 9)]]))
    # the limits of bsg_match_rows_many, once each
    assert "queries" in refused(RawBatch([(T, b"", b"t")], [[term(0)]] * 65))                                                       # 65 queries
    conds64 = [(T, b"", b"t%d" % i) for i in range(63)] + [(R, b"a", b"x")]
    big = [term(i) for i in range(64)] + [_lib.op(_lib.OP_AND, 64)]
    assert "ops" in refused(RawBatch(conds64, [big] * 17))                                                                          # 17 x 127 lowered ops > 2 048
    deep = [term(0)] * 66 + [_lib.op(_lib.OP_OR, 2), _lib.op(_lib.OP_AND, 2)] * 32 + [_lib.op(_lib.OP_OR, 2)]
    assert "deep" in refused(RawBatch(conds64, [[term(63)], deep]))                                                                 # depth 66
    assert "conditions" in refused(RawBatch([(T, b"", b"t%d" % i) for i in range(65)], [[term(0)]]))                                # 65 conditions
    # ... and the plain batched call still refuses a regex kind
    assert "FieldRegex" in refused(RawBatch([(R, b"level", b"err")], [[term(0)]]), ctx.L.bsg_match_rows_many)
    with pytest.raises(BloomGpuError):
        ctx.match_rows_many(rows, RawBatch([(R, b"level", b"err")], [[term(0)]]))
    assert np.array_equal(ctx.device_calls(), before)                                                                              # nothing was launched
    # the context is usable afterwards; the table between the caps runs through the single call, eight of its patterns through the batch
    tall = [('{"f8":"%s"}' % ("ab" * 500)[:lens[8]]).encode(), ('{"f8":"%s"}' % ("c" * (lens[8] - 1))).encode(),
            ('{"f0":"%s"}' % ("0" * lens[0])).encode(), ('{"f5":"%s"}' % ("0" * lens[4])).encode(), b'{"f7":"xyz"}']
    one = Q.CompiledRowQuery(None, Q.RegexOr(*[rx("f%d" % i, "^[0-9a-f]{%d}$" % n) for i, n in enumerate(lens)]))
    got, fb = ctx.match_rows_regex(tall, one)
    assert list(got) == [True, False, True, False, False] and not len(fb)
    planes, fb = ctx.match_rows_many_regex(tall, Q.CompiledRowQueryBatch([(None, rx("f%d" % i, "^[0-9a-f]{%d}$" % lens[i])) for i in range(8)]))
    assert not len(fb) and [int(x) for x in planes.sum(axis=0)] == [0, 0, 1, 0, 0] and planes[0, 2]
    planes, fb = ctx.match_rows_many_regex(rows, Q.CompiledRowQueryBatch([(None, rx("level", "^err")), (Q.FieldToken("level", "error"), None)]))
    assert np.array_equal(planes[0], planes[1]) and planes[0].any() and not len(fb)
    # sixteen regex conditions are within the call
    planes, fb = ctx.match_rows_many_regex([b'{"f3":"x"}'], Q.CompiledRowQueryBatch([(None, rx("f%d" % i, "x|y")) for i in range(16)]))
    assert [int(x) for x in planes[:, 0]] == [int(i == 3) for i in range(16)] and not len(fb)
