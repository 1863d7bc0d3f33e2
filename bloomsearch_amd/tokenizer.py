"""Tokenizers of the separator family (include/bloomgpu.h bsg_tokenizer).

tokens(text) = strings.FieldsFunc(lower ? strings.ToLower(text) : text, isSep): isSep holds for an ASCII rune in
`separators` and, with `unicode_space`, for a rune >= 0x80 with unicode.IsSpace.  Separators are tested after lowering.
Tokenizer.default() is the reference's BasicWhitespaceLowerTokenizer = strings.Fields(strings.ToLower(v)).  Field values
mirror the Go binding's bloomgpu.Tokenizer and the engine JSON's "Tokenizer" object: a missing field is the zero value.

`ngram` is 0 (the words themselves) or 2, 3, 4: a word of more than that many runes is replaced by its windows of that many
consecutive runes, a shorter word stays one token; windows never cross a separator (bloomgpu.h BSG_TOK_NGRAM).  Query tokens
are compared literally; query.Substring / FieldSubstring derive a needle's windows (query.substring_terms).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _lib

WHITE_SPACE = " \t\n\v\f\r"


@dataclass(frozen=True)
class Tokenizer:
    separators: str = ""
    unicode_space: bool = False
    lower: bool = False
    ngram: int = 0

    def __post_init__(self):
        if isinstance(self.ngram, bool) or not isinstance(self.ngram, int) or self.ngram not in (0, 2, 3, 4):
            raise ValueError(f"tokenizer: n-gram width {self.ngram!r} (0, 2, 3 or 4)")
        for ch in self.separators:
            if ch == "\0":
                raise ValueError("tokenizer: NUL cannot be a separator")
            if ord(ch) >= 0x80:
                raise ValueError(f"tokenizer: separator {ch!r} is not ASCII (separators are ASCII only)")

    @classmethod
    def default(cls) -> "Tokenizer":
        return cls(WHITE_SPACE, unicode_space=True, lower=True)

    def sep_ascii(self) -> tuple[int, int]:
        bits = 0
        for ch in self.separators:
            bits |= 1 << ord(ch)
        return bits & (2**64 - 1), bits >> 64

    def to_c(self) -> _lib.Tokenizer:
        t = _lib.Tokenizer()
        t.sep_ascii[0], t.sep_ascii[1] = self.sep_ascii()
        t.flags = (_lib.TOK_UNICODE_SPACE if self.unicode_space else 0) | (_lib.TOK_LOWER if self.lower else 0) | \
            _lib.TOK_NGRAM(self.ngram)
        t.reserved = 0
        return t

    def to_json(self) -> dict:
        """The engine config's "Tokenizer" object (bloomsearch_host.h bse_open)."""
        d = {"Separators": self.separators, "UnicodeSpace": self.unicode_space, "Lower": self.lower}
        if self.ngram:
            d["Ngram"] = self.ngram
        return d


def c_spec(tokenizer) -> "C._Pointer | None":
    """None -> NULL (the default); a Tokenizer or a ready _lib.Tokenizer -> a pointer to its C form."""
    if tokenizer is None:
        return None
    return C.pointer(tokenizer if isinstance(tokenizer, _lib.Tokenizer) else tokenizer.to_c())
