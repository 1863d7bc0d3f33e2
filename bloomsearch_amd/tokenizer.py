"""Tokenizers of the separator family (include/bloomgpu.h bsg_tokenizer).

tokens(text) = strings.FieldsFunc(lower ? strings.ToLower(text) : text, isSep): isSep holds for an ASCII rune in
`separators` and, with `unicode_space`, for a rune >= 0x80 with unicode.IsSpace.  Separators are tested after lowering.
Tokenizer.default() is the reference's BasicWhitespaceLowerTokenizer = strings.Fields(strings.ToLower(v)).  Field values
mirror the Go binding's bloomgpu.Tokenizer and the engine JSON's "Tokenizer" object: a missing field is the zero value.
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

    def __post_init__(self):
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
        t.flags = (_lib.TOK_UNICODE_SPACE if self.unicode_space else 0) | (_lib.TOK_LOWER if self.lower else 0)
        t.reserved = 0
        return t

    def to_json(self) -> dict:
        """The engine config's "Tokenizer" object (bloomsearch_host.h bse_open)."""
        return {"Separators": self.separators, "UnicodeSpace": self.unicode_space, "Lower": self.lower}


def c_spec(tokenizer) -> "C._Pointer | None":
    """None -> NULL (the default); a Tokenizer or a ready _lib.Tokenizer -> a pointer to its C form."""
    if tokenizer is None:
        return None
    return C.pointer(tokenizer if isinstance(tokenizer, _lib.Tokenizer) else tokenizer.to_c())
