"""FieldRegex conditions in the device row matcher (bsg_match_rows_regex: compileRowMatcher's root And(bloom root, regex root),
row_matcher.go:353-573) against two independent answers: the oracle's walker (oracle/walker_oracle.py) for the candidate
texts with Python `re` patterns spelling out RE2's meaning, and the host DFA runner (bsh_regex_match).

Tables: query_test.go:28-30, tokenizer_test.go:193-212, row_matcher_test.go:118-133 / :342 and the regex cases of
no_false_negatives_test.go (user / user.name, a, latency, tags, the empty field).
"""
import re

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q, synth
from bloomsearch_amd.gpu import Context
from oracle import walker_oracle as W
from tests.helpers import device_ids
from tests.test_host_tables import _random_value, go_marshal

pytestmark = pytest.mark.gpu

# pattern -> the same language as a Python `re` pattern (no re flags: RE2's classes, anchors and (?i) orbits spelled out)
PY = {
    "timeout|cache": "timeout|cache",
    "timeout|retry": "timeout|retry",
    "^err": "\\Aerr",
    "^pay": "\\Apay",
    "(?i)error": "[eE][rR][rR][oO][rR]",
    "[0-9]{3}-[0-9]{4}": "[0-9]{3}-[0-9]{4}",
    ".": "[^\\n]",
    "\\Azzz-never-matches\\z": "\\Azzz-never-matches\\Z",
    "^$": "\\A\\Z",
    "a": "a",
    "^[0-9]+$": "\\A[0-9]+\\Z",
    "é|日": "é|日",
    "^true$": "\\Atrue\\Z",
    "(?i)^k": "\\A[kK\u212a]",
    "\\s": "[\\t\\n\\f\\r ]",
    "^-?[0-9]+(\\.[0-9]+)?$": "\\A-?[0-9]+(\\.[0-9]+)?\\Z",
    "b.*a": "b[^\\n]*a",
    "(?i)^jo": "\\A[jJ][oO]",
    "^2$": "\\A2\\Z",
    "Beta": "Beta",
    "region-[37]$": "region-[37]\\Z",
    "(?s)^.*$": "\\A[\\s\\S]*\\Z",
    "x::y|\\?": "x::y|\\?",
    ".*": "[^\\n]*",
    "x": "x",
}
PATTERNS = sorted(PY)


def go_quote_meta(s: str) -> str:
    return "".join("\\" + c if c in "\\.+*?()|[]{}^$" else c for c in s)


def leaves(row: bytes):
    out = []

    def emit(path, value, is_leaf):
        if is_leaf:
            t = W.leaf_token_input(value)
            if t is not None:
                out.append((path, t))
    W.for_each_path_value(W.parse(row), emit)
    return out


def oracle_row(row: bytes, bloom, regex, runner) -> bool:
    """matchRowBytes: the bloom side by the oracle's set matcher, the regex side by compileRegexExpression's rules"""
    if bloom is not None and not W.matches_bloom_expression(row, bloom):
        return False
    lv = leaves(row)

    def cond(c):
        f = c.get("Field", "")
        return any((p == f or p.startswith(f + ".")) and runner(c["Pattern"], t) for p, t in lv)

    def ev(e):
        if e is None:
            return True
        et = e.get("ExpressionType")
        if et == "CONDITION":
            c = e.get("Condition")
            if c is None:
                return True
            if c.get("Field", "") == "":
                return False
            return cond(c)
        kids = e.get("Children") or []
        if et == "OR":
            return any(ev(k) for k in kids)
        if et == "AND":
            return all(ev(k) for k in kids)
        return False
    return ev(regex)


def py_runner(pattern, text):
    return re.search(PY[pattern], text) is not None


def dfa_runner(pattern, text):
    rc = Hst.regex_match(pattern, text)
    assert rc in (0, 1), (pattern, rc)
    return rc == 1


def device(ctx, rows, bloom, regex):
    got, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, regex))
    for r in fb:
        assert not got[r]
    return got, [int(x) for x in fb]


def check(ctx, rows, bloom, regex, runners=(py_runner, dfa_runner)):
    got, fb = device(ctx, rows, bloom, regex)
    for runner in runners:
        want = np.array([oracle_row(r, bloom, regex, runner) for r in rows])
        decided = np.ones(len(rows), dtype=bool)
        decided[fb] = False
        assert np.array_equal(got[decided], want[decided]), (runner.__name__, bloom, regex,
                                                              [rows[i] for i in np.nonzero((got != want) & decided)[0][:3]])
    return got, fb


def test_reference_regex_tables(ctx):
    # query_test.go:28-30
    rx = Q.RegexOr(Q.RegexAnd(Q.FieldRegex("message", "timeout|retry"), Q.FieldRegex("level", "^err")), Q.FieldRegex("service", "^pay"))
    rows = [b'{"level":"error","message":"upstream timeout","service":"auth"}', b'{"level":"info","message":"timeout","service":"auth"}',
            b'{"level":"info","message":"ok","service":"payments"}', b'{"level":"error","message":"ok","service":"auth"}']
    got, fb = check(ctx, rows, None, rx, (dfa_runner,))
    assert list(got) == [True, False, True, False] and not fb
    # tokenizer_test.go:193-212
    rx = Q.RegexAnd(Q.FieldRegex("users.name", "(?i)^jo"), Q.RegexOr(Q.FieldRegex("users.active", "^true$"), Q.FieldRegex("users.id", "^2$")))
    rows = [b'{"users":[{"id":1,"name":"John","active":true},{"id":2,"name":"Jane","active":false}]}',
            b'{"users":[{"id":3,"name":"Alice","active":false}]}']
    got, fb = check(ctx, rows, None, rx)
    assert list(got) == [True, False] and not fb
    # row_matcher_test.go:118-133: bloom + regex, bloom + a regex that never matches, the empty field, a missing field, empty Or
    rows = [go_marshal({"user": {"name": "alice", "id": 7}, "a": "x", "latency": 12.5, "tags": ["Beta gamma", "x::y"]}),
            go_marshal({"user": "bob", "a": {"b": "y"}, "latency": 3, "tags": []})]
    cases = [(Q.Field("user.name"), Q.FieldRegex("user.name", "."), [True, False]),
             (Q.Token("alice"), Q.FieldRegex("user", "\\Azzz-never-matches\\z"), [False, False]),
             (None, Q.FieldRegex("user", "^[0-9]+$"), [True, False]),          # user.id = 7 is beneath "user"
             (None, Q.FieldRegex("a", "."), [True, True]),
             (None, Q.FieldRegex("latency", "^-?[0-9]+(\\.[0-9]+)?$"), [True, True]),
             (None, Q.FieldRegex("tags", "Beta"), [True, False]),              # row_matcher_test.go:342
             (None, Q.FieldRegex("", ".*"), [False, False]),
             (None, Q.FieldRegex("no.such.path", ".*"), [False, False]),
             (None, Q.RegexOr(), [False, False]),
             (None, Q.RegexAnd(), [True, True]),
             (Q.Field("user"), {"ExpressionType": "CONDITION", "Condition": None}, [True, True])]
    for bloom, rx, want in cases:
        got, fb = check(ctx, rows, bloom, rx)
        assert list(got) == want and not fb, (bloom, rx)


def random_rows(seed, n):
    rng = np.random.default_rng(seed)
    rows = [go_marshal({"r": _random_value(rng, 0), **{k: _random_value(rng, 1) for k in ("user", "a", "tags", "a.b")
                                                        if rng.random() < 0.7}}) for _ in range(n)]
    return rows + synth.rows_json(seed * 1000, n)


def random_program(rng, fields):
    def cond():
        return Q.FieldRegex(fields[rng.integers(0, len(fields))], PATTERNS[rng.integers(0, len(PATTERNS))])

    def tree(d):
        if d == 0 or rng.random() < 0.4:
            return cond()
        kids = [tree(d - 1) for _ in range(rng.integers(1, 4))]
        return Q.RegexAnd(*kids) if rng.random() < 0.5 else Q.RegexOr(*kids)
    bloom = [None, Q.Field("user"), Q.Token("alpha"), Q.Or(Q.FieldToken("level", "error"), Q.Field("a")),
             Q.And(Q.Field("message"), Q.Token("cache"))][rng.integers(0, 5)]
    return bloom, tree(2)


def test_random_rows_and_programs(ctx):
    rng = np.random.default_rng(7)
    fields = ["r", "user", "user.name", "a", "a.b", "tags", "message", "level", "service", "nested", "nested.region", "timestamp",
              "user_id", "id", "日本語", "héllo", "x..y", "q?x"]
    total_fb = 0
    for seed in range(4):
        rows = random_rows(seed, 150)
        for _ in range(12):
            bloom, rx = random_program(rng, fields)
            _, fb = check(ctx, rows, bloom, rx)
            total_fb += len(fb)
    assert total_fb < 4 * 12 * 300 // 4


def test_quote_meta_no_false_negatives(ctx):
    rows = random_rows(11, 120)
    for i, row in enumerate(rows):
        lv = leaves(row)
        for path, text in lv:
            rx = Q.FieldRegex(path, "^" + go_quote_meta(text) + "$")
            got, fb = device(ctx, [row], None, rx)
            assert got[0] or fb == [0], (row, path, text)


def test_empty_string_versus_null(ctx):
    rows = [b'{"a":""}', b'{"a":null}', b'{"a":[null,""]}', b'{"a":[null]}']
    got, fb = check(ctx, rows, None, Q.FieldRegex("a", "^$"))
    assert list(got) == [True, False, True, False] and not fb
    got, _ = check(ctx, rows, None, Q.FieldRegex("a", ".*"))
    assert list(got) == [True, False, True, False]


def test_beneath_versus_sibling_prefix(ctx):
    rows = [b'{"ab":"x"}', b'{"a":{"b":"x"}}', b'{"a.b":"x"}', b'{"a":"x"}', b'{"abc":{"a":"x"}}']
    got, fb = check(ctx, rows, None, Q.FieldRegex("a", "x"))
    assert list(got) == [False, True, True, True, False] and not fb


def test_escapes_and_u_runes(ctx):
    row = b'{"m":"tab\\there \\u00e9 \\u65e5 \\ud83d\\ude00 \\n \\"q\\" \\u003c/b\\u003e \xc3\xa9"}'
    for pat, want in [("\\t", True), ("é", True), ("日", True), ("\U0001F600", True), ("\\n", True), ('"q"', True), ("</b>", True),
                      ("^tab\\there é 日 \U0001F600 \\n \"q\" </b> é$", True), ("\\\\", False), ("u00e9", False), ("^.{27}$", False), ("^(?s:.){27}$", True)]:
        got, fb = device(ctx, [row], None, Q.FieldRegex("m", pat))
        assert not fb and bool(got[0]) == want, pat
        assert Hst.regex_match(pat, W.leaf_token_input(W.parse(row)[1][0][1])) == int(want), pat


def test_fallback_rows(ctx):
    long_path = "k" * 100
    rows = [b'{"a":"x\xff"}', ('{"%s":"x"}' % long_path).encode(), b'{"a":"x"}', b'{"a":"y"}']
    got, fb = device(ctx, rows, None, Q.FieldRegex("a", "x"))
    assert fb == [0, 1] and list(got) == [False, False, True, False]
    # more regex conditions on one leaf than a lane holds: handed back, and decided by the host
    rx = Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^x", "x$", "^x$", ".")])
    got, fb = device(ctx, [b'{"a":"x"}', b'{"b":"x"}'], None, rx)
    assert fb == [0] and not got[1]


def test_chunked_and_two_device_calls(ctx):
    rows = synth.rows_json(30000, 6000)
    d = synth.draws(30000, 6000)
    bloom = Q.FieldToken("level", "error")
    rx = Q.RegexOr(Q.FieldRegex("message", "timeout|cache"), Q.FieldRegex("nested.region", "region-[37]$"))
    want = np.array([oracle_row(r, bloom, rx, py_runner) for r in rows])
    assert want.sum() > 100 and (d["level"][want] == synth.LEVELS.index("error")).all()
    got0, fb0 = device(ctx, rows, bloom, rx)
    assert not fb0 and np.array_equal(got0, want)
    try:
        for chunk in (1 << 16, 70001):
            ctx.set_ingest_chunk(chunk)
            got, fb = device(ctx, rows, bloom, rx)
            assert np.array_equal(got, want) and not fb, chunk
            assert ctx.last_match_ms() > 0
    finally:
        ctx.set_ingest_chunk(0)
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        got, fb = device(m, rows, bloom, rx)
        assert np.array_equal(got, want) and not fb


def test_limits(ctx):
    rows = [b'{"a":"x"}']
    with pytest.raises(_lib.BloomGpuError) as e:
        ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, Q.RegexOr(*[Q.FieldRegex("a", "x%d" % i) for i in range(17)])))
    assert e.value.code == _lib.BSG_E_UNSUPPORTED
    got, fb = ctx.match_rows_regex([b'{"f3":"x"}'], Q.CompiledRowQuery(None, Q.RegexOr(*[Q.FieldRegex("f%d" % i, "x|y") for i in range(16)])))
    assert got[0] and not len(fb)
    for pat in ("\\pL", "(a|b)*a(a|b){24}", "(?m)^x", "\\bx"):
        with pytest.raises(_lib.BloomGpuError) as e:
            ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, Q.FieldRegex("a", pat)))
        assert e.value.code == _lib.BSG_E_UNSUPPORTED and "regex condition" in str(e.value)
    # the plain entry point still rejects kind 3
    with pytest.raises(_lib.BloomGpuError) as e:
        ctx.match_rows(rows, Q.CompiledRowQuery(None, Q.FieldRegex("a", "x")))
    assert e.value.code == _lib.BSG_E_INVALID
    # and without regex conditions the new entry point answers like the old one
    rows = synth.rows_json(0, 500)
    e2 = Q.And(Q.FieldToken("level", "error"), Q.Field("nested.az"))
    a, fa = ctx.match_rows(rows, Q.CompiledMatcher(e2))
    b, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(e2, None))
    assert np.array_equal(a, b) and list(fa) == list(fb)


def test_tables_near_the_lds_cap(ctx):
    # ten ~1 000-state DFAs fill ~42.8 KB of the 44 544-byte table budget: the last region and the field strings sit at the top of
    # the blob's 16-bit offsets; an eleventh is over the budget and refused before any launch
    lens = [991 + i for i in range(10)]
    rx = Q.RegexOr(*[Q.FieldRegex("f%d" % i, "^[0-9a-f]{%d}$" % n) for i, n in enumerate(lens)])
    rows = [('{"f9":"%s"}' % ("ab" * 500)[:lens[9]]).encode(), ('{"f9":"%s"}' % ("c" * (lens[9] - 1))).encode(),
            ('{"f0":"%s"}' % ("0" * lens[0])).encode(), ('{"f5":"%s"}' % ("0" * lens[4])).encode(), b'{"f9":"xyz"}']
    got, fb = device(ctx, rows, None, rx)
    assert list(got) == [True, False, True, False, False] and not fb
    assert all(Hst.regex_match("^[0-9a-f]{%d}$" % lens[9], t) == int(w) for t, w in
               [(("ab" * 500)[:lens[9]], True), ("c" * (lens[9] - 1), False)])
    over = Q.RegexOr(*[Q.FieldRegex("f%d" % i, "^[0-9a-f]{%d}$" % (990 + i)) for i in range(11)])
    with pytest.raises(_lib.BloomGpuError) as e:
        ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, over))
    assert e.value.code == _lib.BSG_E_UNSUPPORTED and "LDS" in str(e.value)
