"""The envelope of the device row walker (csrc/ingest.hip.h walker_step: nesting <= 16, paths <= 96 bytes, a 116-byte LDS strip per
lane), restated in plain Python, and named rows at its edges for tests/test_walker_envelope_gpu.py.  tests/test_walker_envelope_shapes.py
keeps this file honest against oracle/walker_oracle.py: every row has the longest path and the depth its entry claims, every family has
rows on both sides, and in_envelope agrees with the claimed side.  Test infrastructure only: nothing below asks the library.

The rule.  in_envelope(row) is true exactly when
  - at most 16 containers are open at once, the root counted, and
  - every member path is at most 96 bytes: the parent's path, a "." when that path is not empty, and the decoded key bytes.
So a 95-byte parent with an empty key is inside ("parent." is 96 bytes) and a 96-byte parent with any member is outside, an empty key
included; a 96-byte path may hold a primitive, an empty container or an array of primitives.  A row outside goes to the host: it is on
the fallback list, a validating ingest has inserted nothing of it, a matcher returns its bit false.

Every row is valid JSON in valid UTF-8 with only the escapes the device decodes: nothing but the envelope can send one to the host.
"""
from __future__ import annotations

import functools
from collections import namedtuple

from oracle import walker_oracle as W

PATH_CAP, MAX_DEPTH = 96, 16

# longest: the longest member path in bytes; depth: the most containers open at once — both by construction, not measured
Shape = namedtuple("Shape", "family name row why longest depth inside")


def measure(row: bytes):
    """(longest member path in bytes, most containers open at once) of the parsed row"""
    longest = depth = 0

    def walk(v, path: bytes, n_open: int):
        nonlocal longest, depth
        if W._is_obj(v):
            depth = max(depth, n_open + 1)
            for key, child in v[1]:
                p = (path + b"." if path else b"") + key.encode("utf-8")
                longest = max(longest, len(p))
                walk(child, p, n_open + 1)
        elif isinstance(v, list):
            depth = max(depth, n_open + 1)
            for child in v:
                walk(child, path, n_open + 1)      # array elements share the array's path

    walk(W.parse(row), b"", 0)
    return longest, depth


def in_envelope(row: bytes) -> bool:
    longest, depth = measure(row)
    return depth <= MAX_DEPTH and longest <= PATH_CAP


# ---- the strings the match conditions of the GPU tests are built from ----
TEXT = "alpha beta"                 # the value under the path rows' longest path (two words)
WORD = "deepword"                   # the word at the deepest leaf of the depth rows
P96 = "a" * 96                      # a one-key path at the cap
SIBLING = "a" * 95 + "z"            # shares P96's first 95 bytes
SIBLING_TEXT = "alpha gamma"
PARENT47, CHILD48 = "b" * 47, "c" * 48          # PARENT47.CHILD48 is 96 bytes
PARENT95 = "d" * 95                 # PARENT95 + "." (an empty key) is 96 bytes
NUMBER = 12345                      # the number under P96 (path_values)
DEEP_CONTAINER = ".".join("a" * 15)             # the path of the 16th object of the all-objects rows (29 bytes)
PREFIX_FIELD = "p.a."               # a dot-split prefix of "a..b" under the parent "p" (and "a." under it whole)


def _obj(*members) -> bytes:
    """members: (key as JSON text, value as JSON text)"""
    return ("{" + ",".join('"%s":%s' % m for m in members) + "}").encode("utf-8")


def _str(text: str) -> str:
    return '"%s"' % text


def nest(kinds: str, leaf: str, key: str = "a") -> bytes:
    """Containers from the root inwards, '{' or '[' each; an object holds the one member `key`."""
    head = "".join('{"%s":' % key if k == "{" else "[" for k in kinds)
    tail = "".join("}" if k == "{" else "]" for k in reversed(kinds))
    return (head + leaf + tail).encode("utf-8")


# the last rune of a key: (name, JSON text, decoded UTF-8 bytes)
LAST_RUNES = [
    ("esc_quote", '\\"', 1), ("u0041", "\\u0041", 1), ("u00e9", "\\u00e9", 2), ("u4e2d", "\\u4e2d", 3), ("ud83d_ude00", "\\ud83d\\ude00", 4),
    ("raw_A", "A", 1), ("raw_e9", "é", 2), ("raw_4e2d", "中", 3), ("raw_1f600", "\U0001F600", 4),
]
PREFIX_KEYS = [(".", "dot"), ("..", "dotdot"), ("a.", "a_dot"), (".a", "dot_a"), ("a..b", "a_dotdot_b"), ("." * 96, "dots96"), ("." * 94, "dots94")]
VALUES = [("string", _str(TEXT), 96, 1), ("number", str(NUMBER), 96, 1), ("true", "true", 96, 1), ("null", "null", 96, 1), ("empty_object", "{}", 96, 2),
          ("empty_array", "[]", 96, 2), ("array_of_primitives", '[1,"alpha",false,null]', 96, 2), ("array_of_empty_object", "[{}]", 96, 3),
          ("array_holding_object", '[{"x":1}]', 98, 3)]


@functools.lru_cache(maxsize=None)
def shapes() -> tuple:
    out = []

    def add(family, name, row, why, longest, depth):
        out.append(Shape(family, name, row, why, longest, depth, longest <= PATH_CAP and depth <= MAX_DEPTH))

    # ---- path length ----
    for n in (95, 96, 97):
        add("path_one_key", "one_key_%d" % n, _obj(("a" * n, _str(TEXT))), "a raw key run against the cap", n, 1)
    add("path_one_key", "sibling_96", _obj((SIBLING, _str(SIBLING_TEXT))), "shares the first 95 bytes of the 96-byte key", 96, 1)
    add("path_one_key", "short", _obj(("a", _str(TEXT))), "far from the cap", 1, 1)
    for parent, letter in ((1, "e"), (47, "b"), (94, "f"), (95, "d"), (96, "g")):
        for total in (95, 96, 97, 98):
            child = total - parent - 1
            if child < 0 or (total == 98 and parent != 96):
                continue
            add("path_two_levels", "parent_%d_child_%d" % (parent, child), _obj((letter * parent, _obj(("c" * child, _str(TEXT))).decode())),
                "the joining dot is byte %d%s" % (parent + 1, ", the key is empty" if child == 0 else ""), total, 2)
    for total in (95, 96, 97):
        add("path_three_levels", "three_levels_%d" % total, _obj(("h" * 30, _obj(("i" * 31, _obj(("j" * (total - 63), _str(TEXT))).decode())).decode())),
            "two joining dots", total, 3)
    for name, text, n in LAST_RUNES:
        for over in range(0, max(n, 2)):           # 0: the key ends at byte 96; then every later start of the rune
            add("path_last_rune", "%s_ends_at_%d" % (name, 96 + over), _obj(("r" * (96 - n + over) + text, _str(TEXT))),
                "the key's last rune (%d bytes) %s" % (n, "ends at the cap" if over == 0 else "straddles or passes the cap"), 96 + over, 1)
    for n in (96, 97):
        add("path_under_parent_rune", "parent_u00e9_%d" % n, _obj(("q", _obj(("s" * (n - 4) + "\\u00e9", _str(TEXT))).decode())),
            "an escaped two-byte rune ends a key under a parent", n, 2)
    for name, value, longest, depth in VALUES:
        add("path_values", "p96_" + name, _obj((P96, value), ("z", _str("after words"))), "a 96-byte path holding: " + name, longest, depth)
    early = (("a", _str("early one")), ("b", _obj(("c", _str("early two"))).decode()), ("d", '[1,2,"early three"]'))
    for n in (96, 97):
        add("path_last_member", "late_key_%d" % n, _obj(*early, ("l" * n, _str(TEXT))),
            "the long key is the LAST member: a walk that does not validate first has emitted already", n, 2)

    # ---- depth ----
    for n in (15, 16, 17):
        add("depth", "objects_%d" % n, nest("{" * n, _str(WORD)), "all objects", 2 * n - 1, n)
        add("depth", "arrays_%d" % n, nest("[" * n, _str(WORD)), "all arrays: no path at all, nothing to emit", 0, n)
        add("depth", "arrays_under_key_%d" % n, nest("{" + "[" * (n - 1), _str(WORD), key="r"), "arrays under one key", 1, n)
        add("depth", "alternating_%d" % n, nest("{[" * (n // 2) + "{" * (n % 2), _str(WORD)), "objects and arrays in turn", 2 * ((n + 1) // 2) - 1, n)
        add("depth", "alternating_array_first_%d" % n, nest("[{" * (n // 2) + "[" * (n % 2), _str(WORD)), "arrays and objects in turn", max(2 * (n // 2) - 1, 0), n)
    reopen = '[{"a":"one"},["two"],{"b":["%s"]}]' % WORD
    add("depth_reopen", "reopen_in_13_arrays", nest("[" * 13, reopen), "depth 16 reached, closed, reached again with the other kind at the same level", 1, 16)
    add("depth_reopen", "reopen_in_14_arrays", nest("[" * 14, reopen), "the same one level deeper", 1, 17)
    add("depth_reopen", "reopen_under_key", nest("{" + "[" * 12, reopen, key="r"), "the same with paths: r, r.a, r.b", 3, 16)
    add("depth_second_member", "objects_16_second_member", nest("{" * 15, '{"a":"first","b":"%s"}' % WORD), "a ',' and a second member at depth 16", 31, 16)
    add("depth_second_member", "arrays_16_second_element", nest("{" + "[" * 15, '"first","%s"' % WORD, key="r"), "a ',' and a second element at depth 16", 1, 16)
    add("depth_second_member", "objects_17_second_member", nest("{" * 16, '{"a":"first","b":"%s"}' % WORD), "the same one level deeper", 33, 17)
    add("depth_late", "late_17", _obj(*early, ("e", nest("{" * 16, _str(WORD)).decode())), "17 containers only after members inside the envelope", 33, 17)
    add("depth_late", "late_16", _obj(*early, ("e", nest("{" * 15, _str(WORD)).decode())), "its twin inside", 31, 16)
    keys = ["m" * 5] * 15 + ["m" * 6]              # 16 keys and 15 dots: 96 bytes
    deep96 = "".join('{"%s":' % k for k in keys) + _str(WORD) + "}" * 16
    add("depth_and_path", "objects_16_path_96", deep96.encode(), "16 containers and a 96-byte path at once", 96, 16)
    add("depth_and_path", "objects_16_path_97", deep96.replace("m" * 6, "m" * 7).encode(), "one byte more", 97, 16)
    add("depth_and_path", "objects_17_path_96", ('{"m":' + deep96.replace("m" * 6, "m" * 4) + "}").encode(), "one container more", 96, 17)

    # ---- key prefixes ----
    for key, name in PREFIX_KEYS:
        add("key_prefixes", "root_" + name, _obj((key, _str(TEXT))), "every dot-split prefix of the key is a field", len(key), 1)
        add("key_prefixes", "parent_" + name, _obj(("p", _obj((key, _str(TEXT))).decode())), "the parent's joining dot is no prefix of its own", len(key) + 2, 2)
    return tuple(out)


def families():
    return sorted({s.family for s in shapes()})


def alignment_rows():
    """[(row, name, longest)] in blob order from offset 0: a raw key of 96 and of 97 bytes behind a filler row, the long row starting at
    each of the eight alignments, so that the 8-byte key scan meets the cap with runs of 1 to 8 bytes."""
    out, at = [], 0
    for n in (96, 97):
        for align in range(8):
            pad = (align - at - 8) % 8             # the filler is 8 + pad bytes long
            out.append((b'{"f":"' + b"x" * pad + b'"}', "filler", 1))
            at += 8 + pad
            row = _obj(("t" * n, _str(TEXT)))
            out.append((row, "key_%d_at_%d" % (n, align), n))
            at += len(row)
    return out


@functools.lru_cache(maxsize=None)
def match_rows() -> tuple:
    """the rows of the match and ingest tests: every shape, then the alignment rows (which need not start at offset 0 to be decided right)"""
    return tuple(s.row for s in shapes()) + tuple(r for r, _, _ in alignment_rows())


# ---- the conditions, built from the shapes ----
Query = namedtuple("Query", "name bloom regex substring range")


def queries(token_of=lambda word: word) -> list:
    """token_of(word): the token a tokenizer makes of a word without separators (an n-gram walker: its first window)."""
    from bloomsearch_amd import query as Q
    rx96, rx_parent, rx_sibling = Q.FieldRegex(P96, "alpha"), Q.FieldRegex(PARENT47, "beta"), Q.FieldRegex(SIBLING, "gamma")
    ft96 = Q.FieldToken(P96, token_of("beta"))
    return [
        Query("field_96", Q.Field(P96), None, None, None),
        Query("field_dot_prefix", Q.Field(PREFIX_FIELD), None, None, None),
        Query("field_container_at_depth_16", Q.Field(DEEP_CONTAINER), None, None, None),
        Query("token_at_the_deepest_leaf", Q.Token(token_of(WORD)), None, None, None),
        Query("field_token_96", ft96, None, None, None),
        Query("or_of_bloom_conditions", Q.Or(Q.Field(PREFIX_FIELD), Q.Token(token_of(WORD)), ft96), None, None, None),
        Query("regex_96", None, rx96, None, None),
        Query("regex_beneath_its_parent", None, rx_parent, None, None),
        Query("regex_beneath_a_95_byte_parent", None, Q.FieldRegex(PARENT95, "alpha"), None, None),
        Query("regex_sibling", None, rx_sibling, None, None),
        Query("or_of_regex_conditions", Q.Token(token_of("alpha")), Q.RegexOr(rx96, rx_parent, rx_sibling), None, None),
        Query("substring_96", None, None, Q.FieldSubstring(P96, "pha be"), None),
        Query("range_96", None, None, None, Q.FieldRange(P96, 12000, 13000)),
        Query("bloom_regex_substring_96", Q.Field(P96), rx96, Q.FieldSubstring(P96, "beta"), None),
        Query("bloom_and_range_96", Q.Token(token_of("after")), None, None, Q.FieldRange(P96, None, 12345)),
    ]


def strip_query(token_of=lambda word: word) -> Query:
    """true on the short rows with k3 and word1 and on the full rows of the letter a — under every subset of its three sides"""
    from bloomsearch_amd import query as Q
    return Query("strip", Q.Or(Q.And(Q.Field("k3.x"), Q.Token(token_of("word1"))), Q.FieldToken("a" * 96, token_of(WORD))),
                 Q.RegexOr(Q.FieldRegex("k3", "^hit$"), Q.FieldRegex("a" * 96, "epwo")),
                 Q.SubstringOr(Q.FieldSubstring("k3.x", "hit"), Q.Substring("epwo")), None)


def token_of(tokenizer=None):
    """word -> its first token under a walker of tests/substring_restatement.WALKERS (None = the default)"""
    from tests import ngram_restatement as NR, substring_restatement as SR
    return lambda word: NR.tokens(word, SR.spec_of(tokenizer))[0].decode("utf-8")


def reference(row: bytes, q: Query, tokenizer=None) -> bool:
    """What a matcher answers for a row it decides: the restatements' verdict of every side, And-ed (tests/ngram_restatement.py with
    tests/tokenizer_restatement.py's regex side, tests/substring_restatement.py, tests/range_restatement.py).  A row outside the
    envelope is the host's: the device's bit for it is false."""
    from tests import ngram_restatement as NR, range_restatement as RR, substring_restatement as SR
    return bool(NR.row_verdict(row, SR.spec_of(tokenizer), q.bloom, q.regex) and SR.row_verdict(row, q.substring, tokenizer) and
                RR.row_verdict(row, q.range))


# ---- strip isolation ----
STRIP_ROWS = 513


def strip_is_full(i: int) -> bool:
    """lane 255 of the first workgroup, lane 0 of the second and the last lane of the launch hold a full row"""
    return i % 2 == 1 if i < 256 else i % 2 == 0


def strip_letter(i: int) -> str:
    return "abcdefghijklmnopqrstuvwxyz"[i % 26]


@functools.lru_cache(maxsize=None)
def strip_rows() -> tuple:
    """Rows that fill their lane's strip — a 96-byte path of one letter (the row's own), 16 containers, fifteen stack entries of 96 —
    alternating with short rows whose verdict hangs on their own first path bytes (k<i % 7>.x) and on a word in a later leaf (word<i % 3>)."""
    rows = []
    for i in range(STRIP_ROWS):
        if strip_is_full(i):
            rows.append(nest("{" + "[" * 15, _str(WORD), key=strip_letter(i) * 96))
        else:
            rows.append(_obj(("k%d" % (i % 7), _obj(("x", _str("hit"))).decode()), ("m", _str("word%d" % (i % 3)))))
    return tuple(rows)
