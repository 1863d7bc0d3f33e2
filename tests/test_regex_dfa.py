"""bsh_regex_match — the DFA compiler / runner behind the device's FieldRegex conditions (host/regex_dfa.hpp) — against
RE2's answers: a known-answer table, the refused constructs, and a seeded fuzz over random pattern ASTs rendered twice,
as RE2 syntax for the library and as Python `re` syntax spelling out RE2's meaning for an independent oracle."""
from __future__ import annotations

import random
import re
import time

import pytest

from bloomsearch_amd import _lib, host

UNSUPPORTED = _lib.BSG_E_UNSUPPORTED


def go_quote_meta(s: str) -> str:
    """regexp.QuoteMeta: a backslash before every one of \\.+*?()|[]{}^$"""
    return "".join("\\" + c if c in "\\.+*?()|[]{}^$" else c for c in s)


KNOWN = [
    ("a$", "a\n", 0), ("\\s", "\v", 0), ("^.$", "é", 1), ("[^a]", "\n", 1),
    ("(?i)k", "K", 1), ("(?i)s", "ſ", 1), ("(?i)i", "ı", 0), ("(?i)K", "K", 1), ("(?i)\\W", "K", 0), ("\\W", "K", 1),
    ("\\d", "٣", 0), ("^$", "", 1), ("\\Azzz-never-matches\\z", "zzz-never-matches", 1), ("\\Azzz-never-matches\\z", "a zzz-never-matches", 0),
    ("timeout|cache", "cache miss on shard 3", 1), ("timeout|cache", "Timeout", 0), ("(?i)error", "an ERROR occurred", 1),
    ("[0-9]{3}-[0-9]{4}", "call 555-0123 now", 1), ("[0-9]{3}-[0-9]{4}", "call 55-0123", 0),
    ("^err", "error", 1), ("^err", "an error", 0), ("^pay", "payments", 1), ("(?i)^jo", "John", 1), ("^true$", "true", 1), ("^2$", "2", 1),
    (".", "\n", 0), ("(?s).", "\n", 1), ("(?s:.)x", "\nx", 1), ("a.c", "aéc", 1), ("^.{3}$", "日本語", 1), ("^.{3}$", "日本", 0),
    ("x*", "", 1), ("$^", "", 1), ("a|", "zzz", 1), ("a(?i)b|c", "C", 1), ("(?i:a)b", "AB", 0), ("(?P<n>ab)+c", "ababc", 1), ("(?<n>x)", "x", 1),
    ("[[:alpha:]]+[[:digit:]]", "abc7", 1), ("[[:^alpha:]]", "abc", 0), ("[^\\d\\s]", "1 2", 0), ("\\x41\\x{1F600}", "A😀", 1),
    ("[\\x{4e00}-\\x{9fff}]", "中", 1), ("a{2,3}?b", "aab", 1), ("a{1000}", "a" * 999, 0), ("a{1000}", "a" * 1000, 1), ("\\v", "\v", 1),
    ("^\\.\\*\\+\\?\\(\\)\\|\\[\\]\\{\\}\\^\\$\\\\$", ".*+?()|[]{}^$\\", 1), ("[]a]", "]", 1), ("[a-]", "-", 1), ("a{,5}", "a{,5}", 1),
    ("(?U)a+", "aaa", 1), ("(?i)[^k]", "K", 0), ("(?i)[k]", "K", 1), ("[^\\n]", "\n", 0),
]

# texts of the reference's property rows (no_false_negatives_test.go, row_matcher_test.go): ^QuoteMeta(text)$ must hit them
PROPERTY_TEXTS = ["John", "Jane", "user-1@example.com", "1E5", "9007199254740993", "-0.5", "true", "false", "", "a.b", "x+y*z",
                  "(paren) [bracket] {brace}", "tab\there", "new\nline", "ünïcödé", "日本語", "😀 emoji", "$100^2", "back\\slash", "Beta gamma"]


@pytest.mark.parametrize("pattern,text,want", KNOWN)
def test_known_answers(pattern, text, want):
    assert host.regex_match(pattern, text) == want, (pattern, text)


@pytest.mark.parametrize("text", PROPERTY_TEXTS)
def test_quote_meta_hits_its_text(text):
    p = "^" + go_quote_meta(text) + "$"
    assert host.regex_match(p, text) == 1
    assert host.regex_match(p, text + "x") == 0


def test_invalid_utf8_text_is_u_fffd_per_byte():
    # Go reads an invalid byte as U+FFFD of width 1: each byte of a truncated sequence is one rune
    assert host.regex_match("^..$", b"\xe2\x82") == 1
    assert host.regex_match("^.$", b"\xff") == 1
    assert host.regex_match("^\\x{FFFD}$", b"\xed\xa0\x80"[:1]) == 1
    assert host.regex_match("^...$", b"\xed\xa0\x80") == 1       # an encoded surrogate is three invalid bytes


@pytest.mark.parametrize("pattern", [
    "\\pL", "\\p{Greek}", "\\PL", "\\bword", "a\\B", "(?m)^a", "\\C", "(?i)é", "(?i)[a-é]", "\\Qa.b\\E", "\\1", "\\Z", "a**", "a+*",
    "*a", "(", "(a", "a)", "[a", "[z-a]", "a{1001}", "a{3,2}", "[[:bogus:]]", "(?x)a", "(?P=n)", "\\e", "\xff",
])
def test_refused(pattern):
    p = pattern.encode("latin-1") if pattern == "\xff" else pattern
    assert host.regex_match(p, "abc") == UNSUPPORTED


def test_state_blowup_is_refused_quickly():
    best = 1e9
    for _ in range(5):                      # the best of a few runs: one sample on a busy machine says little
        t0 = time.perf_counter()
        rc = host.regex_match("(a|b)*a(a|b){24}", "ab")
        best = min(best, time.perf_counter() - t0)
        assert rc == UNSUPPORTED
    assert best < 0.05, best


# ---------------- fuzz: random ASTs over the subset, rendered twice ----------------
ALPHABET = list("abckKsSx019 _-.") + ["\n", "\t", "\v", "é", "ß", "ſ", "K", "中", "😀", "ı", "٣", " "]
SPECIAL = set("\\.+*?()|[]{}^$")
FOLD_EXTRA = {"k": "K", "s": "ſ"}

PERL = {"d": "0-9", "s": "\\t\\n\\f\\r ", "w": "0-9A-Za-z_"}
POSIX = {"alpha": "A-Za-z", "digit": "0-9", "alnum": "0-9A-Za-z", "upper": "A-Z", "lower": "a-z", "space": "\\t\\n\\v\\f\\r ",
         "xdigit": "0-9A-Fa-f", "punct": "!-/:-@\\[-`{-~", "blank": "\\t "}


def orbit(c: str) -> list[str]:
    if c.isascii() and c.isalpha():
        lo = c.lower()
        return [lo, lo.upper()] + ([FOLD_EXTRA[lo]] if lo in FOLD_EXTRA else [])
    return [c]


def py_char(c: str) -> str:
    return "\\U%08x" % ord(c)


def expand_set(items, fold: bool) -> set[str]:
    """the code points of a class's positive items over the ASCII range plus the explicit non-ASCII singles"""
    out = set()
    for it in items:
        if it[0] == "ch":
            out.update(orbit(it[1]) if fold else [it[1]])
        elif it[0] == "rng":
            for o in range(ord(it[1]), ord(it[2]) + 1):
                out.update(orbit(chr(o)) if fold else [chr(o)])
        else:   # perl / posix group: ASCII members
            body = PERL.get(it[1]) or POSIX[it[1]]
            members = [chr(o) for o in range(128) if re.fullmatch("[" + body + "]", chr(o))]
            for m in members:
                out.update(orbit(m) if fold else [m])
    return out


def py_set(chars: set[str], neg: bool) -> str:
    if not chars:
        return "[^\\x00-\\U0010ffff]" if not neg else "[\\x00-\\U0010ffff]"
    return "[" + ("^" if neg else "") + "".join(py_char(c) for c in sorted(chars)) + "]"


class Gen:
    def __init__(self, rng: random.Random):
        self.r = rng

    def char(self, fold: bool) -> str:
        pool = [c for c in ALPHABET if c.isascii()] if fold else ALPHABET
        return self.r.choice(pool)

    def node(self, depth: int, fold: bool, dots: bool):
        r = self.r
        k = r.random()
        if depth <= 0 or k < 0.35:
            return self.leaf(fold, dots)
        if k < 0.55:
            return ("cat", [self.node(depth - 1, fold, dots) for _ in range(r.randint(2, 4))])
        if k < 0.68:
            kids = [self.node(depth - 1, fold, dots) for _ in range(r.randint(2, 3))]
            if r.random() < 0.15:
                kids.append(("empty",))
            return ("alt", kids)
        if k < 0.85:
            q = r.choice(["*", "+", "?", "{n}", "{n,}", "{n,m}"])
            n = r.randint(0, 3)
            m = n + r.randint(0, 2)
            return ("rep", self.node(depth - 1, fold, dots), q, n, m, r.random() < 0.3)
        if k < 0.93:
            f2 = fold or r.random() < 0.5
            d2 = dots or r.random() < 0.5
            return ("flags", "i" if f2 and not fold else "", "s" if d2 and not dots else "", self.node(depth - 1, f2, d2), f2, d2)
        return ("group", r.choice(["(", "(?:", "(?P<g>", "(?<g>"]), self.node(depth - 1, fold, dots))

    def leaf(self, fold: bool, dots: bool):
        r = self.r
        k = r.random()
        if k < 0.45:
            return ("lit", "".join(self.char(fold) for _ in range(r.randint(1, 3))), fold)
        if k < 0.55:
            return ("dot", dots)
        if k < 0.65:
            return ("perl", r.choice("dDsSwW"), fold)
        if k < 0.72:
            return ("anchor", r.choice(["^", "$", "\\A", "\\z"]))
        items = []
        for _ in range(r.randint(1, 3)):
            t = r.random()
            if t < 0.45:
                items.append(("ch", self.char(fold)))
            elif t < 0.7:
                a, b = sorted([r.choice("0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"), r.choice("abcxyzKS")])
                items.append(("rng", a, b))
            elif t < 0.85:
                items.append(("perlc", r.choice("dsw")))
            else:
                items.append(("posix", r.choice(sorted(POSIX))))
        return ("cls", items, r.random() < 0.3, fold)


def re2(n) -> str:
    t = n[0]
    if t == "lit":
        return "".join("\\" + c if c in SPECIAL else ("\\n" if c == "\n" else ("\\t" if c == "\t" else ("\\v" if c == "\v" else c))) for c in n[1])
    if t == "dot":
        return "."
    if t == "perl":
        return "\\" + n[1]
    if t == "anchor":
        return n[1]
    if t == "cls":
        body = ""
        for it in n[1]:
            if it[0] == "ch":
                c = it[1]
                body += "\\" + c if c in SPECIAL or c == "-" else ("\\n" if c == "\n" else c)
            elif it[0] == "rng":
                body += it[1] + "-" + it[2]
            elif it[0] == "perlc":
                body += "\\" + it[1]
            else:
                body += "[:" + it[1] + ":]"
        return "[" + ("^" if n[2] else "") + body + "]"
    if t == "empty":
        return ""
    if t == "cat":
        return "".join(re2(k) if k[0] != "alt" else "(?:" + re2(k) + ")" for k in n[1])
    if t == "alt":
        return "|".join(re2(k) for k in n[1])
    if t == "rep":
        inner = re2(n[1])
        inner = "(?:" + inner + ")" if n[1][0] not in ("lit", "dot", "perl", "cls", "group", "flags") or (n[1][0] == "lit" and len(n[1][1]) > 1) else inner
        q = {"*": "*", "+": "+", "?": "?", "{n}": "{%d}" % n[3], "{n,}": "{%d,}" % n[3], "{n,m}": "{%d,%d}" % (n[3], n[4])}[n[2]]
        return inner + q + ("?" if n[5] else "")
    if t == "flags":
        fl = n[1] + n[2]
        return "(?" + fl + ":" + re2(n[3]) + ")" if fl else "(?:" + re2(n[3]) + ")"
    if t == "group":
        return n[1] + re2(n[2]) + ")"
    raise AssertionError(t)


def py(n) -> str:
    t = n[0]
    if t == "lit":
        return "".join(py_set(set(orbit(c)), False) if n[2] else py_char(c) for c in n[1])
    if t == "dot":
        return "[\\x00-\\U0010ffff]" if n[1] else "[^\\n]"
    if t == "perl":
        c, fold = n[1], n[2]
        return py_set(expand_set([("perlc", c.lower())], fold), c.isupper())
    if t == "anchor":
        return "\\A" if n[1] in ("^", "\\A") else "\\Z"
    if t == "cls":
        items = [(it[0] if it[0] in ("ch", "rng") else "grp",) + it[1:] for it in n[1]]
        return py_set(expand_set(items, n[3]), n[2])
    if t == "empty":
        return ""
    if t == "cat":
        return "".join("(?:" + py(k) + ")" for k in n[1])
    if t == "alt":
        return "|".join("(?:" + py(k) + ")" for k in n[1])
    if t == "rep":
        q = {"*": "*", "+": "+", "?": "?", "{n}": "{%d}" % n[3], "{n,}": "{%d,}" % n[3], "{n,m}": "{%d,%d}" % (n[3], n[4])}[n[2]]
        return "(?:" + py(n[1]) + ")" + q + ("?" if n[5] else "")
    if t == "flags":
        return "(?:" + py(n[3]) + ")"
    if t == "group":
        return "(" + py(n[2]) + ")"
    raise AssertionError(t)


def sample(n, r: random.Random, oracle_cache) -> str:
    """a text the node likely matches (the verdict itself always comes from the oracle)"""
    t = n[0]
    if t == "lit":
        return "".join(r.choice(orbit(c)) if n[2] else c for c in n[1])
    if t in ("dot", "perl", "cls"):
        pat = oracle_cache(py(n))
        cands = [c for c in ALPHABET + ["K", "ſ"] if pat.fullmatch(c)]
        return r.choice(cands) if cands else ""
    if t in ("anchor", "empty"):
        return ""
    if t == "cat":
        return "".join(sample(k, r, oracle_cache) for k in n[1])
    if t == "alt":
        return sample(r.choice(n[1]), r, oracle_cache)
    if t == "rep":
        lo = {"*": 0, "+": 1, "?": 0}.get(n[2], n[3])
        hi = {"*": 3, "+": 3, "?": 1, "{n}": n[3], "{n,}": n[3] + 2}.get(n[2], n[4])
        return "".join(sample(n[1], r, oracle_cache) for _ in range(r.randint(lo, hi)))
    if t == "flags":
        return sample(n[3], r, oracle_cache)
    if t == "group":
        return sample(n[2], r, oracle_cache)
    raise AssertionError(t)


def test_fuzz_against_python_oracle():
    r = random.Random(20261016)
    g = Gen(r)
    cache = {}

    def compiled(p):
        c = cache.get(p)
        if c is None:
            c = cache[p] = re.compile(p)
        return c

    n_patterns = n_hits = n_miss = 0
    failures = []
    while n_patterns < 2000:
        fold = r.random() < 0.1
        ast = g.node(r.randint(1, 4), fold, False)
        if fold:
            ast = ("flags", "i", "", ast, True, False)
        p2 = re2(ast)
        if fold and r.random() < 0.5:
            p2 = "(?i)" + re2(ast[3])   # the leading form of the same flag
        try:
            oracle = compiled(py(ast))
        except re.error as e:
            raise AssertionError(f"test renderer produced bad Python syntax for {p2!r}: {e}")
        texts = []
        for _ in range(3):
            s = sample(ast, r, compiled)
            pre = "".join(r.choice(ALPHABET) for _ in range(r.randint(0, 2)))
            suf = "".join(r.choice(ALPHABET) for _ in range(r.randint(0, 2)))
            texts += [s, pre + s + suf]
            if s:
                i = r.randrange(len(s))
                texts.append(s[:i] + r.choice(ALPHABET) + s[i + 1:])
        texts += ["".join(r.choice(ALPHABET) for _ in range(r.randint(0, 6))) for _ in range(3)]
        n_patterns += 1
        for text in texts:
            want = 1 if oracle.search(text) else 0
            got = host.regex_match(p2, text)
            n_hits += want
            n_miss += 1 - want
            if got != want:
                failures.append((p2, py(ast), text, got, want))
    assert not failures, failures[:10]
    assert n_hits > 3000 and n_miss > 3000, (n_hits, n_miss)
