"""bsg_match_rows_lookup_regex / bsg_match_rows_lookup_regex_rows (k_match_rows_lookup_regex*, k_eval_row_programs_w): the lookup row
matcher over tables of up to 1 024 conditions of which up to 16 distinct ones are FieldRegex.  Expected verdicts come from
tests/test_match_regex_gpu.py's oracle_row with Python `re` as the pattern runner (py_runner; the patterns that file's table does
not spell are spelled here the same way), never from the library, and are compared on decided rows; where a table fits the shipped
wide call the two calls are compared word for word, header for header and fallback list for fallback list; the bit-row call and the
list call of the new family must expand to the same rows."""
import ctypes as C
import re

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q, synth
from bloomsearch_amd.gpu import Context, pack_entries, pair_rows_list, wide_pair_bits
from tests import tokenizer_restatement as TR
from tests.helpers import device_ids
from tests.test_collisions import pair as collision_pair
from tests.test_match_many_gpu import BAD_ROWS, RawBatch, log_queries
from tests.test_match_regex_gpu import PY, oracle_row, py_runner
from tests.test_match_wide_gpu import mixed_items

pytestmark = pytest.mark.gpu

DEEP_ROW = BAD_ROWS[2]                         # nesting depth 17: outside the device walker's envelope
T, FT, R = _lib.KIND_TOKEN, _lib.KIND_FIELD_TOKEN, _lib.KIND_FIELD_REGEX
BIG = "^[0-9a-f]{1000}$"                       # 1 002 DFA states x 2 classes: 4 264 table bytes
# RE2's meaning of the patterns test_match_regex_gpu.PY does not hold, as Python `re` patterns
MORE = {"^a": "\\Aa", "b$": "b\\Z", "x|y": "x|y", "a.*b": "a[^\\n]*b", "[0-9]+": "[0-9]+", BIG: "\\A[0-9a-f]{1000}\\Z"}
assert not set(MORE) & set(PY)


def runner(pattern, text):
    return re.search(MORE[pattern], text) is not None if pattern in MORE else py_runner(pattern, text)


def rx(field, pattern):
    return Q.FieldRegex(field, pattern)


def term(i):
    return [_lib.op(_lib.OP_TERM, i)]


def csr(lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return off, [q for l in lists for q in l]


def oracle_bits(rows, item):
    bloom, regex = item if isinstance(item, tuple) else (item, None)
    return np.array([oracle_row(r, bloom, regex, runner) for r in rows], dtype=bool)


def both_calls(ctx, rows, batch, first=None, lists=None, tokenizer=None):
    """both calls of the family -> (per pair bool row from the bits, fallback rows, the bit call's result, the list call's); the
    lists must expand to the same rows"""
    if first is None:
        sets, args = [(0, len(rows))] * (len(batch.prog_off) - 1), ()
    else:
        off, flat = csr(lists)
        sets, args = [(first[s], first[s + 1]) for s, l in enumerate(lists) for _ in l], (first, off, flat)
    bits_result = ctx.match_rows_lookup_regex(rows, batch, *args, tokenizer=tokenizer)
    rows_result = ctx.match_rows_lookup_regex_rows(rows, batch, *args, tokenizer=tokenizer)
    words, pwo, fb = bits_result
    hdr, poff, payload, fb_rows = rows_result
    assert len(pwo) - 1 == len(sets) == len(hdr) and fb.tobytes() == fb_rows.tobytes()
    out = []
    for p, (lo, hi) in enumerate(sets):
        bits = wide_pair_bits(words, pwo, p, hi - lo)
        listed = pair_rows_list(int(hdr[p]), payload[int(poff[p]): int(poff[p + 1])], hi - lo)
        assert np.array_equal(np.flatnonzero(bits), listed), p
        out.append(bits)
    return out, [int(r) for r in fb], bits_result, rows_result


def equal_to_the_wide_calls(ctx, rows, batch, first, lists, tokenizer=None):
    """-> both_calls' result, after the byte-for-byte comparison with bsg_match_rows_wide / _wide_rows over the same table"""
    assert len(batch.kinds) <= 64
    args = () if first is None else (first,) + csr(lists)
    got = both_calls(ctx, rows, batch, first, lists, tokenizer)
    wide = ctx.match_rows_wide(rows, batch, *args, tokenizer=tokenizer)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(wide, got[2]))
    wide_rows = ctx.match_rows_wide_rows(rows, batch, *args, tokenizer=tokenizer)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(wide_rows, got[3]))
    return got


def test_equals_the_wide_calls(ctx):
    rows = synth.rows_json(500, 300)
    items = mixed_items(70)
    batch = Q.CompiledLookupRegexBatch(items)
    wide_batch = Q.CompiledWideBatch(items)
    assert (batch.kinds, batch.fields, batch.tokens, batch.prog_ops) == (wide_batch.kinds, wide_batch.fields, wide_batch.tokens, wide_batch.prog_ops)
    assert len(batch.kinds) <= 64 and batch.kinds.count(R) == 3
    first = [0, 100, 200, 300]
    rng = np.random.default_rng(70)
    uneven = [sorted(int(q) for q in rng.choice(70, size=n, replace=False)) for n in (1, 37, 70)]
    regex_queries = [q for q in range(70) if isinstance(items[q], tuple)]
    assert len(regex_queries) >= 3
    total = 0
    for lists in ([list(range(70))] * 3, uneven, [list(range(70)), [], regex_queries]):
        out, fb, _, _ = equal_to_the_wide_calls(ctx, rows, batch, first, lists)
        assert fb == []                                                                # on these rows the wide tests hand back no row either
        p = 0
        for s, listed in enumerate(lists):
            for q in listed:
                if q in regex_queries[:3] or q in (0, 9):                             # the oracle on the regex pairs, a log query and a wide Or
                    assert np.array_equal(out[p], oracle_bits(rows[first[s]: first[s + 1]], items[q])), (s, q)
                    total += int(out[p].sum())
                p += 1
    assert total > 0 and ctx.last_match_ms() > 0


def test_set_masks_open_the_dfas(ctx):
    pats = ["timeout|cache", "timeout|retry", "b.*a", "a", "x"]                        # five regex conditions on one field: a lane holds four
    items = [(None, rx("message", p)) for p in pats] + [(Q.FieldToken("level", "error"), rx("message", "a")), Q.FieldToken("service", "auth")]
    rows = synth.rows_json(100, 300)
    for r, text in ((5, b'{"level":"info"}'), (130, b'{"message":null}'), (250, b'{"msg":"timeout"}')):
        rows[r] = text
    batch = Q.CompiledLookupRegexBatch(items)
    assert batch.kinds.count(R) == 5
    first = [0, 100, 200, 300]
    want = [oracle_bits(rows, e) for e in items]

    def check(lists, tokenizer=None, queries=range(len(items))):
        out, fb, _, _ = equal_to_the_wide_calls(ctx, rows, batch, first, lists, tokenizer)
        p = 0
        for s, listed in enumerate(lists):
            decided = np.array([r not in fb for r in range(first[s], first[s + 1])])
            for q in listed:
                if q in queries:
                    assert np.array_equal(out[p][decided], want[q][first[s]: first[s + 1]][decided]), (s, q)
                assert not out[p][~decided].any()
                p += 1
        return out, fb

    out, fb = check([[0, 1, 2, 5, 6], [1, 2, 3, 4, 6], [0, 4]])
    assert not fb and sum(int(o.sum()) for o in out) > 50                              # at most four of the five per set: nothing handed back
    out, fb = check([[0, 1, 2, 5, 6], [0, 1, 2, 3, 4], [0, 4]])
    assert fb == [r for r in range(100, 200) if r != 130]                              # the set that uses all five: its rows with a message text
    spec = TR.SPECS["punct_lower"]                                                     # the _tok instance; the regex-only queries read no word
    out, fb = check([[0, 5, 6], [], [3, 5, 6]], tokenizer=spec, queries=range(5))
    assert not fb and sum(int(o.sum()) for o in out) > 20


BOUNDARY = [(63, b"ra", b"^a", "abc", "cba"), (64, b"rb", b"b$", "ab", "ba"), (127, b"rc", b"x|y", "wxw", "wzw"), (128, b"rd", b"a.*b", "a--b", "b--a"),
            (1023, b"re", b"[0-9]+", "v12", "vv")]                                     # table index, field, pattern, a text it matches, one it does not


def boundary_case(n_conds):
    at = [b for b in BOUNDARY if b[0] < n_conds]
    conds = [(T, b"", b"t%d" % c) for c in range(n_conds)]
    for c, field, pattern, _, _ in at:
        conds[c] = (R, field, pattern)
    tok_a, tok_b = 70, n_conds - 3                                                     # Token conditions of the second and of the last word
    AND, OR = _lib.op(_lib.OP_AND, 2), _lib.op(_lib.OP_OR, 2)
    programs, want = [], []                                                            # want: the verdict from the per-condition truths
    for b in at:
        programs.append(term(b[0]))
        want.append(lambda v, c=b[0]: v[c])
    for i, a in enumerate(at):
        for b in at[i + 1:]:
            programs += [term(a[0]) + term(b[0]) + [AND], term(a[0]) + term(b[0]) + [OR]]
            want += [lambda v, x=a[0], y=b[0]: v[x] & v[y], lambda v, x=a[0], y=b[0]: v[x] | v[y]]
    programs += [term(at[0][0]) + term(tok_a) + [AND], term(at[-1][0]) + term(tok_b) + [OR], term(tok_a) + term(at[1][0]) + [OR] + term(tok_b) + [AND]]
    want += [lambda v: v[at[0][0]] & v[tok_a], lambda v: v[at[-1][0]] | v[tok_b], lambda v: (v[tok_a] | v[at[1][0]]) & v[tok_b]]
    return at, conds, programs, want, (tok_a, tok_b)


def boundary_rows(at, toks, n_rows):
    rows = []
    for r in range(n_rows):                                                            # every subset of the boundary conditions, and the two tokens
        doc = {field.decode(): (hit if (r >> k) & 1 else miss) for k, (_, field, _, hit, miss) in enumerate(at)}
        words = ["t%d" % toks[0]] * (r % 3 == 0) + ["t%d" % toks[1]] * (r % 5 < 2) + ["zz"]
        rows.append(('{"m":"%s",%s}' % (" ".join(words), ",".join('"%s":"%s"' % kv for kv in doc.items()))).encode())
    return rows


@pytest.mark.parametrize("n_rows", [1, 64, 65, 257])
@pytest.mark.parametrize("n_conds", [129, 1024])
def test_word_boundaries(ctx, n_conds, n_rows):
    at, conds, programs, want, toks = boundary_case(n_conds)
    assert len(at) == (5 if n_conds == 1024 else 4) and len(conds) == n_conds
    rows = boundary_rows(at, toks, n_rows)
    out, fb, _, _ = both_calls(ctx, rows, RawBatch(conds, programs))
    assert not fb
    truth = {c: oracle_bits(rows, (None, rx(field.decode(), pattern.decode()))) for c, field, pattern, _, _ in at}
    truth.update({c: oracle_bits(rows, Q.Token("t%d" % c)) for c in toks})
    for q, w in enumerate(want):
        assert np.array_equal(out[q], w(truth)), q
    if n_rows >= 64:
        assert all(truth[c].any() and not truth[c].all() for c in truth)


def test_identity_at_the_limit(ctx):
    n = 1024
    exprs = [Q.FieldToken("f%d" % i, "t%d" % i) for i in range(1008)] + [(None, rx("r%d" % j, "x|y")) for j in range(16)]
    rows = [b'{"f%d":"t%d"}' % (i, i) for i in range(1008)] + [b'{"r%d":"%s"}' % (j, b"xy"[j & 1: (j & 1) + 1]) for j in range(16)]
    batch = Q.CompiledLookupRegexBatch(exprs)
    assert len(batch.kinds) == n and batch.n_queries == n and batch.kinds.count(FT) == 1008 and batch.kinds.count(R) == 16
    before = ctx.device_calls().sum()
    words, pwo, fb = ctx.match_rows_lookup_regex(rows, batch)
    assert ctx.device_calls().sum() == before + 1 and len(fb) == 0 and ctx.last_match_ms() > 0   # strings and pairs at their maximum: the cap is 19 456
    got = np.unpackbits(words.view(np.uint8).reshape(n, n // 8), axis=1, bitorder="little").astype(bool)
    assert np.array_equal(got, np.eye(n, dtype=bool))                                  # pair i matches exactly row i
    hdr, poff, payload, fb = ctx.match_rows_lookup_regex_rows(rows, batch)
    assert len(fb) == 0 and all(int(h) == (2 << 30 | 1) for h in hdr)                  # BSG_ROW_LIST, one row
    assert [int(x) for x in payload] == list(range(n)) and [int(x) for x in poff] == list(range(n + 1))
    sample = [0, 1, 63, 64, 1007, 1008, 1009, 1022, 1023]
    for q in (0, 1007, 1008, 1015, 1023):                                              # the oracle on a few queries
        assert np.array_equal(got[q][sample], oracle_bits([rows[r] for r in sample], exprs[q])), q


def test_repeated_conditions(ctx):
    same = (R, b"message", b"timeout|cache")
    conds = [(T, b"", b"error"), same, same] + [(R, b"o%d" % i, b"x|y") for i in range(15)] + [same] * 17 + [(T, b"", b"warn"), same]
    where = [c for c, x in enumerate(conds) if x == same]
    assert len(where) == 20 and len([x for x in conds if x[0] == R]) == 35             # 16 distinct regex conditions
    rows = synth.rows_json(300, 130) + [b'{"o7":"y","message":"no"}', b'{"o7":"z"}']
    batch = RawBatch(conds, [term(c) for c in where] + [term(3 + 7), term(0)])
    out, fb, _, _ = both_calls(ctx, rows, batch)
    assert not fb
    want = oracle_bits(rows, (None, rx("message", "timeout|cache")))
    assert want.any() and not want.all()
    for q in range(20):
        assert np.array_equal(out[q], want), q
    assert list(np.flatnonzero(out[20])) == [130] and np.array_equal(out[21], oracle_bits(rows, Q.Token("error")))


def raw_call(ctx, rows, batch, rows_call):
    """the C call itself, with tables the Python layer would refuse to build"""
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
        rc = ctx.L.bsg_match_rows_lookup_regex_rows(*head, p(hdr), None, p(bits), 2 * total, C.byref(length), p(fb), len(fb), C.byref(nfb))
    else:
        rc = ctx.L.bsg_match_rows_lookup_regex(*head, p(bits), p(fb), len(fb), C.byref(nfb))
    assert rc == _lib.BSG_OK or not bits.any()
    return rc


@pytest.mark.parametrize("rows_call", [False, True])
def test_refusals(ctx, rows_call):
    rows = synth.rows_json(0, 70)
    U = _lib.BSG_E_UNSUPPORTED
    message = lambda: ctx.L.bsg_last_error(ctx.h).decode()
    full = [(FT, b"f%d" % i, b"t%d" % i) for i in range(1008)]
    six = [(R, b"field_%d" % i, BIG.encode()) for i in range(6)]                       # 6 x 4 287 bytes of tables
    refused = [(RawBatch([(R, b"f%d" % i, b"x") for i in range(17)], [term(16)]), ("17 regex conditions", "16")),
               (RawBatch([(T, b"", b"t"), (R, b"a", b"\\bx")], [term(0)]), ("regex condition 1", "\\bx")),
               (RawBatch([(T, b"", b"t%d" % i) for i in range(1024)] + [(R, b"a", b"x")], [term(0)]), ("1025 conditions", "1024")),
               (RawBatch(full + six, [term(1008)]), ("19456 bytes of LDS",))]
    for batch, words in refused:
        before = ctx.device_calls()
        assert raw_call(ctx, rows, batch, rows_call) == U
        assert all(w in message() for w in words), message()
        assert np.array_equal(ctx.device_calls(), before), words                       # refused before any launch
    # the context still works: sixteen distinct regex conditions run, and the same six tables over ten Token conditions are accepted
    before = ctx.device_calls().sum()
    assert raw_call(ctx, rows, RawBatch([(R, b"f%d" % i, b"x") for i in range(16)] + [(R, b"f3", b"x")], [term(16)]), rows_call) == _lib.BSG_OK
    tall = [b'{"field_0":"%s"}' % (b"0" * 1000), b'{"field_0":"%s"}' % (b"0" * 999), b'{"field_3":"%s","k":"t4"}' % (b"ab" * 500),
            b'{"field_5":"%s"}' % (b"c" * 1001), b'{"field_1":"%s"}' % (b"g" * 1000), b'{"k":"t4 t9"}']
    items = [Q.Token("t%d" % i) for i in range(10)] + [(None, rx("field_%d" % i, BIG)) for i in range(6)] + [(Q.Token("t4"), rx("field_3", BIG))]
    batch = Q.CompiledLookupRegexBatch(items)
    assert len(batch.kinds) == 16
    if rows_call:
        hdr, poff, payload, fb = ctx.match_rows_lookup_regex_rows(tall, batch)
        got = [pair_rows_list(int(hdr[q]), payload[int(poff[q]): int(poff[q + 1])], len(tall)) for q in range(len(items))]
    else:
        words, pwo, fb = ctx.match_rows_lookup_regex(tall, batch)
        got = [np.flatnonzero(wide_pair_bits(words, pwo, q, len(tall))) for q in range(len(items))]
    assert not len(fb) and ctx.device_calls().sum() == before + 2
    for q, e in enumerate(items):
        assert list(got[q]) == list(np.flatnonzero(oracle_bits(tall, e))), q
    assert list(got[10]) == [0] and list(got[13]) == [2] and list(got[16]) == [2] and not len(got[15]) and not len(got[11])


def test_fallback_rows_and_sets_without_pairs(ctx):
    a, b = collision_pair(3)
    colliding = b'{"k":"' + a + b'"}'                                                  # emits a token with the hashes of condition b, not its bytes
    good = [b'{"k":"t%d","msg":"%s"}' % (i, b"abc" if i % 2 else b"cba") for i in range(20)]
    rows = good + [DEEP_ROW, colliding] + good + [DEEP_ROW, colliding]
    conds = [(T, b"", b"t%d" % i) for i in range(99)] + [(T, b"", b), (R, b"msg", b"^a")]   # condition 99: the collision partner, in a role it has
    batch = RawBatch(conds, [term(3), term(99), [], term(100)])
    first = [0, 22, 44]
    off, flat = csr([[0, 1, 2, 3], []])
    words, pwo, fb = ctx.match_rows_lookup_regex(rows, batch, first, off, flat)
    assert [int(r) for r in fb] == [20, 21]                                            # handed back where listed; the set without pairs is not walked
    assert list(np.flatnonzero(wide_pair_bits(words, pwo, 0, 22))) == [3]
    assert not wide_pair_bits(words, pwo, 1, 22).any()
    assert np.array_equal(wide_pair_bits(words, pwo, 2, 22), np.arange(22) < 20)       # nil expression: every decided row; the handed-back rows' bits are 0
    assert np.array_equal(wide_pair_bits(words, pwo, 3, 22), oracle_bits(good, (None, rx("msg", "^a"))).tolist() + [False, False])
    out, fb, _, _ = both_calls(ctx, rows, batch)
    assert fb == [20, 21, 42, 43] and np.array_equal(out[3][:20], out[3][22:42]) and out[3][:20].sum() == 10
    # the collision partner as a regex condition's FIELD has no role a word is compared in: such a row is decided
    out, fb, _, _ = both_calls(ctx, [colliding, good[1]], RawBatch([(R, b, b"^a"), (R, b"msg", b"^a")], [term(0), term(1)]))
    assert not fb and not out[0].any() and list(out[1]) == [False, True]


def test_a_regex_free_table_is_the_lookup_call(ctx):
    exprs = [Q.Token("t%d" % i) for i in range(200)]
    rows = [b'{"k":"t%d t%d"}' % (i % 210, (i * 7) % 230) for i in range(300)]
    rows[77], rows[256] = DEEP_ROW, BAD_ROWS[0]
    batch, plain = Q.CompiledLookupRegexBatch(exprs), Q.CompiledLookupBatch(exprs)
    assert batch.kinds == plain.kinds and batch.prog_ops == plain.prog_ops
    first = [0, 100, 100, 300]
    lists = [list(range(200)), list(range(0, 200, 3)), list(range(100, 200))]
    off, flat = csr(lists)
    for args in ((), (first, off, flat)):
        got, want = ctx.match_rows_lookup_regex(rows, batch, *args), ctx.match_rows_lookup(rows, plain, *args)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and got[0].any() and [int(r) for r in got[2]] == [77, 256]
        got, want = ctx.match_rows_lookup_regex_rows(rows, batch, *args), ctx.match_rows_lookup_rows(rows, plain, *args)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and len(got[2]) > 0


def test_chunks_and_devices(ctx):
    n_rows = 20000
    rows = synth.rows_json(7000, n_rows)
    where = [0, 63, 64, 6999, 7000, n_rows - 1]
    for i, r in enumerate(where):
        rows[r] = BAD_ROWS[i % len(BAD_ROWS)]
    d = synth.draws(7000, n_rows)
    regex_items = [(Q.FieldToken("level", "error"), rx("message", "timeout|cache")), (None, rx("service", "^pay")), (Q.Token("timeout"), rx("level", "^err"))]
    others = log_queries(30, 7000) + [Q.Token("error"), Q.Field("nested.az"), None]
    n_other = len(Q.CompiledLookupRegexBatch(others + regex_items).kinds)
    users = sorted(set(int(x) for x in d["user_id"]))[: 129 - n_other]
    items = [Q.FieldToken("user_id", str(u)) for u in users] + others + regex_items
    batch = Q.CompiledLookupRegexBatch(items)
    assert len(batch.kinds) == 129 and batch.kinds.count(R) == 3
    nq = batch.n_queries
    first = [0, 7000, 7000, n_rows]
    lists = [list(range(nq)), list(range(nq)), sorted(set(range(0, nq, 3)) | {nq - 2})]
    off, flat = csr(lists)
    w0, p0, f0 = ctx.match_rows_lookup_regex(rows, batch, first, off, flat)
    r0 = ctx.match_rows_lookup_regex_rows(rows, batch, first, off, flat)
    assert [int(r) for r in f0] == where and f0.tobytes() == r0[3].tobytes()
    sample = [r for r in range(1, 400) if r not in where]                              # the oracle on the regex queries, first set
    for q in (nq - 3, nq - 2, nq - 1):
        bits = wide_pair_bits(w0, p0, q, 7000)
        want = oracle_bits([rows[r] for r in sample], items[q])
        assert np.array_equal(bits[sample], want), q
        assert np.array_equal(np.flatnonzero(bits), pair_rows_list(int(r0[0][q]), r0[2][int(r0[1][q]): int(r0[1][q + 1])], 7000)) and bits.any()
    try:
        ctx.set_ingest_chunk(1 << 16)                                                  # the smallest chunk: tens of launches, sets cut by them
        w1, p1, f1 = ctx.match_rows_lookup_regex(rows, batch, first, off, flat)
        r1 = ctx.match_rows_lookup_regex_rows(rows, batch, first, off, flat)
    finally:
        ctx.set_ingest_chunk(0)
    assert w1.tobytes() == w0.tobytes() and f1.tobytes() == f0.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(r0, r1))
    for n_dev in (1, 2, 3):
        with Context(device_ids(n_dev)) as m:                                          # aliases of one device
            m.set_lab(7, 1)                                                            # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            w2, p2, f2 = m.match_rows_lookup_regex(rows, batch, first, off, flat)
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            r2 = m.match_rows_lookup_regex_rows(rows, batch, first, off, flat)
        assert w2.tobytes() == w0.tobytes() and p2.tobytes() == p0.tobytes() and f2.tobytes() == f0.tobytes(), n_dev
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r0, r2)), n_dev
