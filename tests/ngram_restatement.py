"""A Python restatement of the n-gram tokens of a separator-family spec (include/bloomgpu.h BSG_TOK_NGRAM), the expected
values of the n-gram tests.  It is built on tests/tokenizer_restatement.py (decode_runes, tokens, leaves) and
oracle/walker_oracle.py; it never asks the library under test.

    tokens(text) = concat over w in FieldsFunc(lower ? ToLower(text) : text, isSep) of grams(w, n)

grams(w, n): with o_0 < ... < o_L = len(w) the byte offsets of w's runes as Go's `range` decodes them (an invalid byte is one
rune of width 1), [w] if L <= n, else w[o_i : o_(i+n)] for i = 0 .. L - n.
"""
from bloomsearch_amd.tokenizer import Tokenizer
from tests import tokenizer_restatement as R

NOSEP = ""
SPECS = {
    "tri_default": Tokenizer(R.WHITE_SPACE, unicode_space=True, lower=True, ngram=3),
    "bi_punct_raw": Tokenizer(R.PUNCT, unicode_space=True, lower=False, ngram=2),
    "four_nosep_raw": Tokenizer(NOSEP, ngram=4),
    "four_nosep_lower": Tokenizer(NOSEP, lower=True, ngram=4),
}


def grams(w: bytes, n: int) -> list:
    offs = [0]
    for _, raw in R.decode_runes(w):
        offs.append(offs[-1] + len(raw))
    L = len(offs) - 1
    if L <= n:
        return [w]
    return [w[offs[i]:offs[i + n]] for i in range(L - n + 1)]


def tokens(text, spec: Tokenizer) -> list:
    """-> list of bytes; a spec of width 0 gives tokenizer_restatement.tokens."""
    words = R.tokens(text, spec)
    if not spec.ngram:
        return words
    return [g for w in words for g in grams(w, spec.ngram)]


def entry_sets(rows, spec: Tokenizer, sets=None):
    """bloomEntrySets.indexRow under spec -> (fields, tokens, field_tokens), sets of str."""
    fields, toks, fts = sets if sets is not None else (set(), set(), set())
    for row in rows:
        for path, is_leaf, text in R.leaves(row):
            fields.add(path)
            if text is None:
                continue
            for t in tokens(text, spec):
                ts = t.decode("utf-8", "surrogatepass")
                toks.add(ts)
                fts.add(path + "::" + ts)
    return fields, toks, fts


def row_tokens(row, spec: Tokenizer) -> list:
    """every token of the row's leaves, in walk order (the matcher tests draw their condition tokens from these)"""
    return [t for _, _, text in R.leaves(row) if text is not None for t in tokens(text, spec)]


def row_verdict(row, spec: Tokenizer, bloom=None, regex=None) -> bool:
    """compileRowMatcher's root And(bloom, regex) on one row: Field = a path is emitted, Token = a token of the spec anywhere,
    FieldToken = the (path, token) pair at one leaf; the regex side reads the leaf text and is tokenizer_restatement's."""
    ls = R.leaves(row)
    paths = {p for p, _, _ in ls}
    words, pairs = set(), set()
    for p, _, text in ls:
        if text is None:
            continue
        for t in tokens(text, spec):
            words.add(t)
            pairs.add((p, t))

    def ev(e):
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
            return all([ev(x) for x in kids])
        if et == "OR":
            return any([ev(x) for x in kids])
        return False

    return ev(bloom) and R.row_verdict(row, spec, None, regex)
