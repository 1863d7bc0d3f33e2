"""A Python restatement of the separator-family tokenizers (include/bloomgpu.h bsg_tokenizer), the expected values of the
tokenizer tests.  It is built on oracle/walker_oracle.py (for_each_path_value, leaf_token_input, _to_lower_rune) and a
literal unicode.IsSpace list; it never asks the library under test.

    tokens(text) = strings.FieldsFunc(lower ? strings.ToLower(text) : text, isSep)

Runes are decoded as Go decodes a string: an invalid byte is (U+FFFD, width 1).  strings.ToLower writes U+FFFD for it;
without lowering FieldsFunc keeps the raw byte inside its word.
"""
import re

from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from oracle import walker_oracle as W

# unicode.IsSpace (Go, White_Space): written out, not taken from the oracle or the library
IS_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] +
                     list(range(0x2000, 0x200B)))

PUNCT = " \t\n\v\f\r,;:=/.-\"[]()"
SPECS = {
    "punct_lower": Tokenizer(PUNCT, unicode_space=True, lower=True),
    "punct_raw": Tokenizer(PUNCT, unicode_space=True, lower=False),
    "comma_semi": Tokenizer(",;"),
    "default_plus_01": Tokenizer(WHITE_SPACE + "\x01", unicode_space=True, lower=True),
}


def _utf8_len(b0: int) -> int:
    if b0 < 0x80:
        return 1
    if 0xC2 <= b0 < 0xE0:
        return 2
    if 0xE0 <= b0 < 0xF0:
        return 3
    if 0xF0 <= b0 < 0xF5:
        return 4
    return 0


def decode_runes(b: bytes):
    """utf8.DecodeRune over b: yields (rune, raw bytes); an invalid or truncated sequence is (0xFFFD, one byte)."""
    i = 0
    while i < len(b):
        n = _utf8_len(b[i])
        if n:
            try:
                ch = b[i:i + n].decode("utf-8", "strict")
                if len(ch) == 1 and i + n <= len(b):
                    yield ord(ch), b[i:i + n]
                    i += n
                    continue
            except UnicodeDecodeError:
                pass
        yield 0xFFFD, b[i:i + 1]
        i += 1


def tokens(text, spec: Tokenizer) -> list:
    """FieldsFunc(lower ? ToLower(text) : text, isSep) -> list of bytes."""
    b = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else text
    out, cur = [], bytearray()
    for r, raw in decode_runes(b):
        if spec.lower:
            r = ord(W._to_lower_rune(chr(r)))
        sep = (r < 0x80 and chr(r) in spec.separators) or (r >= 0x80 and spec.unicode_space and r in IS_SPACE)
        if sep:
            if cur:
                out.append(bytes(cur))
                cur = bytearray()
        elif spec.lower:
            cur += chr(r).encode("utf-8")
        else:
            cur += raw
    if cur:
        out.append(bytes(cur))
    return out


def _go_text(s: str) -> str:
    """encoding/json writes U+FFFD for a lone surrogate escape"""
    return "".join("\ufffd" if 0xD800 <= ord(c) <= 0xDFFF else c for c in s)


def leaves(row):
    """[(path, is_leaf, text or None)] in walk order (walker_oracle.for_each_path_value + leaf_token_input)."""
    out = []

    def emit(path, value, is_leaf):
        text = W.leaf_token_input(value) if is_leaf else None
        out.append((path, is_leaf, None if text is None else _go_text(text)))

    W.for_each_path_value(W.parse(row), emit)
    return out


def entry_sets(rows, spec: Tokenizer, sets=None):
    """bloomEntrySets.indexRow under spec -> (fields, tokens, field_tokens), sets of str."""
    fields, toks, fts = sets if sets is not None else (set(), set(), set())
    for row in rows:
        for path, is_leaf, text in leaves(row):
            fields.add(path)
            if text is None:
                continue
            for t in tokens(text, spec):
                ts = t.decode("utf-8", "surrogatepass")
                toks.add(ts)
                fts.add(path + "::" + ts)
    return fields, toks, fts


def row_verdict(row, spec: Tokenizer, bloom=None, regex=None) -> bool:
    """compileRowMatcher's root And(bloom, regex) on one row: Field = a path is emitted, Token = a word anywhere,
    FieldToken = the (path, word) pair at one leaf; FieldRegex = re.search of the pattern on the text of a leaf at or under
    the field (patterns are kept to syntax where Python re and RE2 agree)."""
    ls = leaves(row)
    paths = {p for p, _, _ in ls}
    words, pairs = set(), set()
    for p, is_leaf, text in ls:
        if text is None:
            continue
        for t in tokens(text, spec):
            words.add(t)
            pairs.add((p, t))

    def bloom_ev(e):
        if e is None:
            return True
        et = e.get("ExpressionType")
        if et == "CONDITION":
            c = e.get("Condition")
            if c is None:
                return True
            t, f, k = c.get("Type"), c.get("Field", ""), c.get("Token", "").encode("utf-8", "surrogatepass")
            if t == "FIELD":
                return f in paths
            if t == "TOKEN":
                return k in words
            if t == "FIELD_TOKEN":
                return (f, k) in pairs
            return False
        kids = e.get("Children") or []
        if et == "AND":
            return all([bloom_ev(x) for x in kids])
        if et == "OR":
            return any([bloom_ev(x) for x in kids])
        return False

    def regex_ev(e):
        if e is None:
            return True
        et = e.get("ExpressionType")
        if et == "CONDITION":
            c = e.get("Condition")
            if c is None:
                return True
            f = c.get("Field", "")
            if f == "":
                return False
            rx = re.compile(c["Pattern"])
            return any(text is not None and (p == f or p.startswith(f + ".")) and rx.search(text) for p, _, text in ls)
        kids = e.get("Children") or []
        if et == "AND":
            return all([regex_ev(x) for x in kids])
        if et == "OR":
            return any([regex_ev(x) for x in kids])
        return False

    return bloom_ev(bloom) and regex_ev(regex)
