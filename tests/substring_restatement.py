"""A Python restatement of the substring conditions (include/bloomgpu.h "Substring conditions"), the expected values of the
substring tests.  Built on tests/tokenizer_restatement.py (decode_runes, leaves) and oracle/walker_oracle.py's one-rune lower
table; it never asks the library under test and never calls str.lower.

    fold(x) = strings.ToLower(x) under a spec with lower, else x
    Substring(needle): some leaf's candidate text T has fold(needle) in fold(T); FieldSubstring(field, needle): a leaf whose path
    equals the field.
"""
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from oracle import walker_oracle as W
from tests import tokenizer_restatement as TR

DEFAULT = Tokenizer.default()
TRIGRAM = Tokenizer(WHITE_SPACE, unicode_space=True, lower=True, ngram=3)
PUNCT = TR.SPECS["punct_lower"]
RAW = Tokenizer(WHITE_SPACE, unicode_space=True, lower=False)
WALKERS = {"default": None, "separators": PUNCT, "trigram": TRIGRAM}      # the three device walkers (None = the default kernels)


def spec_of(tokenizer) -> Tokenizer:
    return DEFAULT if tokenizer is None else tokenizer


def fold(text, spec: Tokenizer) -> bytes:
    b = text.encode("utf-8", "surrogatepass") if isinstance(text, str) else text
    if not spec.lower:
        return b
    return b"".join(W._to_lower_rune(chr(r)).encode("utf-8") for r, _ in TR.decode_runes(b))


def runes(b: bytes) -> list:
    return [raw for _, raw in TR.decode_runes(b)]


def row_verdict(row, sub, tokenizer=None) -> bool:
    """The substring tree on one row: nil expression / condition true, empty Or false, empty And true, unknown node false."""
    spec = spec_of(tokenizer)
    texts = [(p, fold(t, spec)) for p, is_leaf, t in TR.leaves(row) if is_leaf and t is not None]

    def ev(e):
        if e is None:
            return True
        et = e.get("ExpressionType")
        if et == "CONDITION":
            c = e.get("Condition")
            if c is None:
                return True
            needle, field = fold(c["Needle"], spec), c.get("Field")
            return any(needle in t for p, t in texts if field is None or p == field)
        kids = e.get("Children") or []
        if et == "AND":
            return all([ev(x) for x in kids])
        if et == "OR":
            return any([ev(x) for x in kids])
        return False
    return ev(sub)
