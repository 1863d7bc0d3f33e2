"""The row matchers under a spec with an n-gram width (the _gram and _regex_gram walkers of the four families): the device's bits,
with the rows it hands back decided by the host matcher under the same spec, equal the Python restatement's verdicts
(tests/ngram_restatement.py) on every row for bsg_match_rows_tok; the same batch through bsg_match_rows_many, _many_regex, _wide,
_wide_rows, _lookup and _lookup_regex agrees with the single call query for query and fallback row for fallback row; a spec
whose width field is 0 returns what it returns without the field."""
import functools
import random

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from bloomsearch_amd.tokenizer import Tokenizer
from tests import ngram_restatement as G, tokenizer_restatement as R
from tests.test_tokenizer_ingest_gpu import FALLBACK_ROWS
from tests.test_tokenizer_match_gpu import FIELDS as WORD_FIELDS, regex_expr
from tests.test_tokenizer_ngram_ingest_gpu import row_sets

pytestmark = pytest.mark.gpu

FIELDS = WORD_FIELDS + ["w", "two", "three", "four", "stroke", "k", "long", "pp", "o", "t", "f", "z", "arr", "deep.a.b", "one", "emo", "mixed"]


@functools.lru_cache(maxsize=None)
def all_rows():
    rows = [r for s in row_sets() for r in s]
    random.Random(17).shuffle(rows)
    return rows


@functools.lru_cache(maxsize=None)
def rows_and_pool(name):
    """the rows, and the condition tokens of a spec: real windows of the rows, whole short words, near misses (a window with its
    last rune replaced, a window one rune short, a window plus the rune that follows it)"""
    spec = G.SPECS[name]
    rows = all_rows()
    r = random.Random("pool-" + name)
    pool = []
    for row in r.sample(rows, 60):
        toks = G.row_tokens(row, spec)
        for t in r.sample(toks, min(3, len(toks))):
            try:
                s = t.decode("utf-8")
            except UnicodeDecodeError:
                continue
            pool.append(s)
            runes = list(s)
            if len(runes) == spec.ngram:
                pool.append("".join(runes[:-1]) + "q")
                pool.append("".join(runes[:-1]))
                pool.append(s + "e")
    pool += ["ok", "a", "x", "be", "é", "日", "😀", "😀😁😂😃", "hello", "alice", "true", "tru", "rue", "-1.", "kel", "Kel", "ab ", " ab", "abc", "abcd"]
    return rows, sorted(set(pool))


def cond(r, pool):
    t = r.choice(["FIELD", "TOKEN", "FIELD_TOKEN", "TOKEN"])
    c = {"Type": t}
    if t != "TOKEN":
        c["Field"] = r.choice(FIELDS)
    if t != "FIELD":
        c["Token"] = r.choice(pool)
    return {"ExpressionType": "CONDITION", "Condition": c}


def expr(r, pool, depth=0):
    if depth >= 2 or r.random() < 0.4:
        return cond(r, pool)
    return {"ExpressionType": r.choice(["AND", "OR"]), "Children": [expr(r, pool, depth + 1) for _ in range(r.randint(1, 3))]}


def decided(rows, spec, bits, fb, bloom, regex=None):
    """the device's bits with the handed-back rows decided by the host matcher under the same spec"""
    assert not bits[fb].any()
    got = bits.copy()
    for i in fb:
        row = rows[int(i)]
        got[i] = Hst.match_row(bloom, row, spec) and (regex is None or Hst.match_row_regex(regex, row))
    return got


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_match_rows_tok_matches_the_restatement(ctx, name):
    spec = G.SPECS[name]
    rows, pool = rows_and_pool(name)
    r = random.Random(name)
    hits = 0
    for _ in range(25):
        bloom = expr(r, pool)
        want = np.array([G.row_verdict(x, spec, bloom) for x in rows])
        bits, fb = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=spec)
        assert set(fb.tolist()) >= {i for i, x in enumerate(rows) if x in FALLBACK_ROWS}
        assert len(fb) < len(rows) // 4                     # the device decides the rest, or nearly: the host matcher is not the one under test
        got = decided(rows, spec, bits, fb, bloom)
        assert np.array_equal(got, want), (name, bloom, np.flatnonzero(got != want)[:5])
        hits += int(want.any() and not want.all())
    assert hits >= 5                                        # a property of the inputs alone: one program in five, at least, tells rows apart


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_match_rows_tok_with_regex_conditions(ctx, name):
    spec = G.SPECS[name]
    rows, pool = rows_and_pool(name)
    r = random.Random("regex-" + name)
    for _ in range(12):
        bloom, regex = (expr(r, pool) if r.random() < 0.8 else None), regex_expr(r)
        want = np.array([G.row_verdict(x, spec, bloom, regex) for x in rows])
        bits, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex), tokenizer=spec)
        assert len(fb) >= len(FALLBACK_ROWS)
        got = decided(rows, spec, bits, fb, bloom, regex)
        assert np.array_equal(got, want), (name, bloom, regex, np.flatnonzero(got != want)[:5])


def pairs_as_bits(hdr, pair_off, payload, n_queries, n_rows):
    out = np.zeros((n_queries, n_rows), dtype=bool)
    for q in range(n_queries):
        out[q, pair_rows_list(hdr[q], payload[int(pair_off[q]): int(pair_off[q + 1])], n_rows)] = True
    return out


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_the_families_agree_with_the_single_call(ctx, name):
    """six plain queries through _many, _wide, _wide_rows and _lookup, six (bloom, regex) queries through _many_regex, _wide and
    _lookup_regex: every plane equals the single call's bits for that query, every fallback list the union of the single calls'"""
    spec = G.SPECS[name]
    rows, pool = rows_and_pool(name)
    n = len(rows)
    r = random.Random("families-" + name)
    plain = [expr(r, pool) for _ in range(6)]
    rx_pool = [regex_expr(r) for _ in range(2)]             # <= 4 distinct regex conditions: a leaf never holds more than a lane's slots,
    mixed = [(expr(r, pool) if r.random() < 0.8 else None, r.choice(rx_pool)) for _ in range(6)]   # in the batch as in the single call

    one = [ctx.match_rows(rows, Q.CompiledMatcher(b), tokenizer=spec) for b in plain]
    want = np.array([h for h, _ in one], dtype=bool)
    want_fb = sorted(set(int(i) for _, fb in one for i in fb))
    assert want.any() and len(want_fb) >= len(FALLBACK_ROWS)

    def same(what, bits, fb, want_bits=None, want_rows=None):
        assert np.array_equal(np.asarray(bits, dtype=bool), want if want_bits is None else want_bits), (name, what)
        assert [int(i) for i in fb] == (want_fb if want_rows is None else want_rows), (name, what)

    planes, fb = ctx.match_rows_many(rows, Q.CompiledMatcherBatch(plain), tokenizer=spec)
    same("many", planes, fb)
    words, pwo, fb = ctx.match_rows_wide(rows, Q.CompiledWideBatch(plain), tokenizer=spec)
    same("wide", [wide_pair_bits(words, pwo, q, n) for q in range(6)], fb)
    hdr, poff, payload, fb = ctx.match_rows_wide_rows(rows, Q.CompiledWideBatch(plain), tokenizer=spec)
    same("wide_rows", pairs_as_bits(hdr, poff, payload, 6, n), fb)
    words, pwo, fb = ctx.match_rows_lookup(rows, Q.CompiledLookupBatch(plain), tokenizer=spec)
    same("lookup", [wide_pair_bits(words, pwo, q, n) for q in range(6)], fb)

    one = [ctx.match_rows_regex(rows, Q.CompiledRowQuery(b, x), tokenizer=spec) for b, x in mixed]
    rx_want = np.array([h for h, _ in one], dtype=bool)
    rx_fb = sorted(set(int(i) for _, fb in one for i in fb))
    planes, fb = ctx.match_rows_many_regex(rows, Q.CompiledRowQueryBatch(mixed), tokenizer=spec)
    same("many_regex", planes, fb, rx_want, rx_fb)
    words, pwo, fb = ctx.match_rows_wide(rows, Q.CompiledWideBatch(mixed), tokenizer=spec)
    same("wide regex", [wide_pair_bits(words, pwo, q, n) for q in range(6)], fb, rx_want, rx_fb)
    words, pwo, fb = ctx.match_rows_lookup_regex(rows, Q.CompiledLookupRegexBatch(mixed), tokenizer=spec)
    same("lookup_regex", [wide_pair_bits(words, pwo, q, n) for q in range(6)], fb, rx_want, rx_fb)


def test_width_0_matches_what_the_spec_without_the_field_matches(ctx):
    spec = R.SPECS["punct_lower"]
    t = spec.to_c()
    t.flags |= _lib.TOK_NGRAM(0)
    rows, pool = rows_and_pool("tri_default")
    r = random.Random(5)
    from tests.test_tokenizer_match_gpu import expr as word_expr
    for _ in range(10):
        bloom, regex = word_expr(r), regex_expr(r)
        a = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=spec)
        b = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tokenizer=t)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), bloom
        a = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex), tokenizer=spec)
        b = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex), tokenizer=t)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (bloom, regex)


def test_a_substring_query_is_the_and_of_the_needle_windows(ctx):
    """the header's rule: the trigram spec finds "imeou" inside "error:timeout" as ime AND meo AND eou, which no word tokenizer can"""
    rows = [b'{"msg":"error:timeout"}', b'{"msg":"time out"}', b'{"msg":"IMEOU"}', b'{"msg":"im eou"}']
    needle = Q.And(Q.Token("ime"), Q.Token("meo"), Q.Token("eou"))
    got, fb = ctx.match_rows(rows, Q.CompiledMatcher(needle), tokenizer=G.SPECS["tri_default"])
    assert got.tolist() == [True, False, True, False] and len(fb) == 0
    got, fb = ctx.match_rows(rows, Q.CompiledMatcher(needle))
    assert not got.any()


def test_the_device_refuses_other_widths(ctx):
    rows = [b'{"msg":"abcdef"}']
    m = Q.CompiledMatcher(Q.Token("abc"))
    for width in (1, 5, 6, 7):
        t = Tokenizer.default().to_c()
        t.flags |= width << _lib.TOK_NGRAM_SHIFT
        with pytest.raises(BloomGpuError) as e:
            ctx.match_rows(rows, m, tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID and "width %d" % width in str(e.value)
        with pytest.raises(BloomGpuError) as e:
            ctx.match_rows_lookup(rows, Q.CompiledLookupBatch([Q.Token("abc")]), tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID
    got, fb = ctx.match_rows(rows, m, tokenizer=G.SPECS["tri_default"])
    assert got.tolist() == [True] and len(fb) == 0
