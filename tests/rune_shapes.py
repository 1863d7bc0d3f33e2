"""The rune path of the device walkers (csrc/ingest.hip.h: S_STR_UTF8, the \\uXXXX and surrogate states, rune_utf8, str_rune and its
0x20000-entry lower table, gram_push; csrc/match.hip.h: SubLane::feed_rune) as shape families with expected values in closed form, for
tests/test_rune_edges_gpu.py.  tests/test_rune_shapes.py keeps this file honest: the closed forms against tests/tokenizer_restatement.py,
tests/ngram_restatement.py, tests/substring_restatement.py and the host mirror, the pinned counts, the fallback rule, the coverage of
gram_push's cases by a replay of its arithmetic.  Test infrastructure only: nothing below asks the library.

Closed forms.  lower(cp) is oracle/walker_oracle._to_lower_rune.  A row {"v":"x<cp>y"} under a spec has the token x + l + y with
l = lower(cp) under a lowering spec and cp otherwise — or, where l is a separator of the spec, the tokens x and y; a row {"v":"<cp>"} has
the token l, or none.  (Words of three runes are their own n-gram at the widths used here, 3 and 4.)

The two conditions on fallback lists.
  1. Under a spec with lower (the default tokenizer included) a row is handed back exactly when one of its string values holds a code
     point of UNKNOWN: below U+20000, unassigned in Unicode 13.0.0, not in a Unicode 14.0 case pair or among the uncased letters 14.0
     added beside them (A7D3, A7D5, A7F2..A7F4), no noncharacter (FDD0..FDEF, xFFFE, xFFFF) and outside 1F000..1FBFF (pictographs,
     never cased).  634 ranges, 44 137 code points, committed as tests/golden/unicode13_unassigned.json and re-derived from unicodedata
     where the interpreter has Unicode 13.0.0.
  2. Under a spec without lower no table is read: the list is empty.
Rows of the families below are valid JSON in valid UTF-8 inside the walker's envelope, so nothing else hands one back; family F's rows
are handed back for the one fault each names.
"""
from __future__ import annotations

import functools
import itertools
import json
import os
import unicodedata
from collections import namedtuple

from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from oracle import walker_oracle as W
from tests import ngram_restatement as NR
from tests import tokenizer_restatement as TR
from tests import walker_envelope_shapes as ENV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unicode13_unassigned.json")
TABLE_END = 0x20000                                  # the lower table's size: a code point at or above it is never looked up
PATH_CAP = ENV.PATH_CAP

N_PAIRS = 1407
LENGTH_HISTOGRAM = {(2, 2): 440, (3, 3): 682, (4, 4): 260, (3, 2): 21, (2, 3): 2, (2, 1): 1, (3, 1): 1}
N_UNKNOWN_RANGES, N_UNKNOWN = 634, 44137

UTF8_EDGES = [0x80, 0x7FF, 0x800, 0xFFF, 0x1000, 0xCFFF, 0xD000, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF,
              0x10000, 0x1FFFF, 0x20000, 0x2FFFF, 0x3FFFF, 0x40000, 0xFFFFF, 0x100000, 0x10FFFF]
SPACES = sorted(c for c in TR.IS_SPACE if c >= 0x80)                  # 19: 85, A0, 1680, 2000..200A, 2028, 2029, 202F, 205F, 3000


def lower(cp: int) -> int:
    return ord(W._to_lower_rune(chr(cp)))


def utf8(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def escaped(cp: int, upper: bool) -> bytes:
    """\\uXXXX, a surrogate pair at or above U+10000; hex digits in one letter case"""
    fmt = "\\u%04X" if upper else "\\u%04x"
    if cp < 0x10000:
        return (fmt % cp).encode()
    v = cp - 0x10000
    return (fmt % (0xD800 + (v >> 10)) + fmt % (0xDC00 + (v & 0x3FF))).encode()


@functools.lru_cache(maxsize=None)
def case_pairs() -> tuple:
    """((cp, lower(cp))) for every code point the oracle lowers to another one: found by iteration"""
    return tuple((cp, lower(cp)) for cp in range(0x80, 0x110000) if not 0xD800 <= cp <= 0xDFFF and lower(cp) != cp)


def length_changing() -> list:
    return [cp for cp, lo in case_pairs() if len(utf8(cp)) != len(utf8(lo))]


# ---- the unknown code points ----
KNOWN_14_UNCASED = (0xA7D3, 0xA7D5, 0xA7F2, 0xA7F3, 0xA7F4)


def ranges_of(cps) -> list:
    out = []
    for cp in cps:
        if out and out[-1][1] == cp - 1:
            out[-1][1] = cp
        else:
            out.append([cp, cp])
    return out


def derive_unknown_ranges() -> list:
    """the rule of the module docstring over this interpreter's unicodedata (meaningful at Unicode 13.0.0 only)"""
    in_pair = {c for p in case_pairs() for c in p}
    return ranges_of(cp for cp in range(0x80, TABLE_END)
                     if unicodedata.category(chr(cp)) == "Cn" and cp not in in_pair and cp not in KNOWN_14_UNCASED
                     and not 0xFDD0 <= cp <= 0xFDEF and (cp & 0xFFFE) != 0xFFFE and not 0x1F000 <= cp <= 0x1FBFF)


@functools.lru_cache(maxsize=None)
def unknown_ranges() -> tuple:
    return tuple((int(a), int(b)) for a, b in json.load(open(GOLDEN))["ranges"])


@functools.lru_cache(maxsize=None)
def unknown_set() -> frozenset:
    return frozenset(cp for a, b in unknown_ranges() for cp in range(a, b + 1))


def is_unknown(cp: int) -> bool:
    return cp in unknown_set()


# ---- the specs ----
DEFAULT = Tokenizer.default()
K_SEP = Tokenizer(WHITE_SPACE + "k", unicode_space=True, lower=True)      # U+212A lowers to a separator
I_SEP = Tokenizer(WHITE_SPACE + "i", unicode_space=True, lower=True)      # U+0130 lowers to a separator
# name -> (the spec whose rule applies, the tokenizer argument of the calls: None = the default kernels)
SPECS = {
    "default": (DEFAULT, None),
    "punct_lower": (TR.SPECS["punct_lower"],) * 2,
    "punct_raw": (TR.SPECS["punct_raw"],) * 2,
    "k_sep": (K_SEP,) * 2,
    "i_sep": (I_SEP,) * 2,
    "tri_default": (NR.SPECS["tri_default"],) * 2,
    "four_nosep_lower": (NR.SPECS["four_nosep_lower"],) * 2,
}
A_SPECS = sorted(SPECS)
B_SPECS = ["default", "punct_lower", "tri_default"]


def is_sep(r: int, spec: Tokenizer) -> bool:
    return (r < 0x80 and chr(r) in spec.separators) or (r >= 0x80 and spec.unicode_space and r in TR.IS_SPACE)


def word_tokens(cps, spec: Tokenizer) -> list:
    """the closed form for a string of code points: lower each under a lowering spec, split at separators, windows of spec.ngram runes"""
    out, cur = [], []
    for cp in list(cps) + [None]:
        r = None if cp is None else (lower(cp) if spec.lower else cp)
        if r is None or is_sep(r, spec):
            if cur:
                n = spec.ngram
                grams = [cur] if not n or len(cur) <= n else [cur[i:i + n] for i in range(len(cur) - n + 1)]
                out += ["".join(chr(c) for c in g) for g in grams]
            cur = []
        else:
            cur.append(r)
    return out


def hands_back(cps, spec: Tokenizer) -> bool:
    """condition 1 and 2 of the module docstring, on the code points of a row's string values"""
    return spec.lower and any(is_unknown(cp) for cp in cps)


# A row with what is expected of it under any spec: `cps` are the code points of its one string value "v" (key "v" unless `key`)
Row = namedtuple("Row", "row cps name key")


def make_row(body: bytes, cps, name: str, key: bytes = b"v") -> Row:
    return Row(b'{"' + key + b'":"' + body + b'"}', tuple(cps), name, key.decode())


# ---- family A: the code-point sweep ----
@functools.lru_cache(maxsize=None)
def sweep_code_points() -> tuple:
    cps = set()
    for cp, lo in case_pairs():
        cps |= {cp, lo}
    cps |= set(UTF8_EDGES)
    for a, b in ranges_of(SPACES):
        cps |= set(range(a - 1, b + 2))
    for a, b in unknown_ranges():
        cps |= {a - 1, a, b, b + 1}
    return tuple(sorted(cp for cp in cps if not 0xD800 <= cp <= 0xDFFF))


def sweep_rows(cps) -> list:
    """four rows per code point: mid-word and alone, raw and escaped (upper-case hex mid-word, lower-case alone)"""
    X, Y = ord("x"), ord("y")
    out = []
    for cp in cps:
        out.append(make_row(b"x" + utf8(cp) + b"y", (X, cp, Y), "U+%04X mid raw" % cp))
        out.append(make_row(b"x" + escaped(cp, True) + b"y", (X, cp, Y), "U+%04X mid escaped" % cp))
        out.append(make_row(utf8(cp), (cp,), "U+%04X alone raw" % cp))
        out.append(make_row(escaped(cp, False), (cp,), "U+%04X alone escaped" % cp))
    return out


A_CHUNK = 1536                                       # code points per ingest call: 6 144 rows, 24 sets of 64 code points


def sweep_chunks() -> list:
    cps = sweep_code_points()
    return [cps[i:i + A_CHUNK] for i in range(0, len(cps), A_CHUNK)]


# ---- family B: byte phase ----
B_RUNES = [0xE9, 0x4E2D, 0x1F600]                    # 2, 3 and 4 bytes; none cased, a space or unknown
RUN_A, RUN_B = b"abcdefghij", b"klmnopqrstu"         # ASCII runs of 10 and 11 bytes


def phase_rows(start: int = 0) -> list:
    """[(Row, offset of the rune's first byte in the rows' blob, phase wanted)], the rows laid end to end from offset `start`: the key is
    `pad` letters so that the rune's first byte falls at the wanted phase of the 8-byte words the walker reads."""
    out, at = [], start
    for cp in B_RUNES:
        for spell in ("raw", "escaped"):
            text = utf8(cp) if spell == "raw" else escaped(cp, cp == 0x4E2D)
            for place in ("first", "last", "between"):
                for phase in range(8):
                    head, tail = {"first": (b"", b"z"), "last": (b"w", b""), "between": (RUN_A, RUN_B)}[place]
                    pad = (phase - (at + 2 + 3 + len(head)) - 1) % 8 + 1     # {" key ":" head; the key is never empty
                    key = b"k" * pad
                    cps = tuple(head) + (cp,) + tuple(tail)
                    r = make_row(head + text + tail, cps, "U+%04X %s %s phase %d" % (cp, spell, place, phase), key)
                    out.append((r, at + 2 + pad + 3 + len(head), phase))
                    at += len(r.row)
    return out


def alone_phase_row(cp: int, phase: int, spell: str = "raw") -> Row:
    """a row that is the whole buffer, its string ending on the rune whose first byte is at `phase`"""
    text = utf8(cp) if spell == "raw" else escaped(cp, False)
    pad = (phase - (2 + 3 + 1) - 1) % 8 + 1
    return make_row(b"w" + text, (ord("w"), cp), "U+%04X %s alone in the buffer phase %d" % (cp, spell, phase), b"k" * pad)


# ---- family C: the n-gram ring ----
ASCII_ALPHABET = [ord(c) for c in "abcdefghijklmnopqrstuvwxyz0123456789"]


def _plain(cps):
    return [cp for cp in cps if lower(cp) == cp and cp not in TR.IS_SPACE and not is_unknown(cp) and unicodedata.category(chr(cp)) != "Cn"]


@functools.lru_cache(maxsize=None)
def alphabets() -> dict:
    """runes of each UTF-8 length that no spec changes: not cased, no space, assigned"""
    return {1: ASCII_ALPHABET, 2: _plain(range(0xDF, 0x250)), 3: _plain(range(0x4E00, 0x5200)), 4: _plain(range(0x1F300, 0x1F500)) + _plain(range(0x20000, 0x20200))}


RING_SPECS = {2: Tokenizer(TR.PUNCT, unicode_space=True, lower=False, ngram=2), 3: NR.SPECS["tri_default"], 4: NR.SPECS["four_nosep_lower"]}


@functools.lru_cache(maxsize=None)
def ring_words(n: int) -> tuple:
    """every word of n + 2 runes over the byte lengths {1, 2, 3, 4}: (lengths, code points); the rune at position j of word w is drawn
    from the alphabet of its length at an index that depends on (w, j), advanced until every window of the word is new"""
    alpha, seen, out = alphabets(), set(), []
    for w, lens in enumerate(itertools.product((1, 2, 3, 4), repeat=n + 2)):
        for k in itertools.count():
            cps = tuple(alpha[L][(w * 7 + j * 13 + k * (31 + j)) % len(alpha[L])] for j, L in enumerate(lens))
            wins = [cps[i:i + n] for i in range(3)]
            if len(set(wins)) == 3 and not any(x in seen for x in wins):
                break
        seen.update(wins)
        out.append((lens, cps))
    return tuple(out)


def ring_rows(n: int) -> list:
    return [make_row(b"".join(utf8(c) for c in cps), cps, "n=%d lengths %s" % (n, "".join(map(str, lens))), b"w") for lens, cps in ring_words(n)]


def ring_replay(lens, n: int) -> set:
    """gram_push's arithmetic over the byte lengths of one word's runes -> the cases it passes through"""
    cases, cnt, tot, q = set(), 0, 0, []
    for L in lens:
        if cnt == n:
            cases.add(("drop", q[0]))
            tot -= q.pop(0)
            cnt -= 1
        cases.add(("fill", tot))
        if tot < 8:
            cases.add(("lo",) if tot + L <= 8 else ("straddle", tot))
        else:
            cases.add(("hi",))
        q.append(L)
        cnt += 1
        tot += L
        if cnt == n and tot == 16:
            cases.add(("window16",))
    return cases


RING_CASES = {("drop", l) for l in (1, 2, 3, 4)} | {("fill", t) for t in range(13)} | {("lo",), ("hi",), ("window16",)} | {("straddle", t) for t in (5, 6, 7)}

LOWERED = [0x23A, 0x1E9E, 0x212A, 0x130]             # 2 -> 3, 3 -> 2, 3 -> 1, 2 -> 1 bytes when lowered


def lowered_words(n: int) -> list:
    """words of n + 2 runes over the four code points whose length changes when lowered and an ASCII capital ('A' + position): all 5^5
    for n = 3, every seventh of the 5^6 for n = 4"""
    words = [tuple(LOWERED[s] if s < 4 else ord("A") + j for j, s in enumerate(sym)) for sym in itertools.product(range(5), repeat=n + 2)]
    return words if n == 3 else words[::7]


def lowered_rows(n: int) -> list:
    return [make_row(b"".join(utf8(c) for c in cps), cps, "lowered n=%d %s" % (n, " ".join("%04X" % c for c in cps)), b"w") for cps in lowered_words(n)]


# ---- family D: the text consumers ----
def four_byte_block_ends() -> list:
    """both ends of every run of four-byte case pairs"""
    return sorted({c for a, b in ranges_of(cp for cp, _ in case_pairs() if cp >= 0x10000) for c in (a, b)})


def consumer_code_points() -> list:
    return sorted(set(length_changing()) | {0x130} | set(four_byte_block_ends()))


def substring_rows() -> list:
    """[(Row, needle that matches, needle that must not)]: {"t":"ab<CP>cd"} raw and escaped; the needles are lower-case"""
    out = []
    for cp in consumer_code_points():
        lo = lower(cp)
        near = lo + 1 if lower(lo + 1) == lo + 1 and lo + 1 >= 0x80 else lo - 1
        cps = (ord("a"), ord("b"), cp, ord("c"), ord("d"))
        for spell, text in (("raw", utf8(cp)), ("escaped", escaped(cp, True))):
            out.append((make_row(b"ab" + text + b"cd", cps, "U+%04X %s" % (cp, spell), b"t"), "b" + chr(lo) + "c", "b" + chr(near) + "c"))
    return out


REGEX_CODE_POINTS = [0xC9, 0x416, 0x1E9E, 0x212A, 0x10400, 0x1E900, 0x23A, 0x2C62]      # two of each length with case pairs, and two more


# ---- family E: runes in keys ----
def key_rows() -> list:
    """[(row, field that must match, field that must not)]: the key <CP>k raw and escaped"""
    out = []
    for cp in (0xC9, 0x416, 0x212A, 0x1E9E, 0x10400, 0x1E900):
        for text in (utf8(cp), escaped(cp, True), escaped(cp, False)):
            out.append((b'{"' + text + b'k":"value"}', chr(cp) + "k", chr(lower(cp)) + "k"))
    return out


def key_cap_rows() -> list:
    """[(row, longest path, field)]: keys of cap - n and cap - n + 1 ASCII bytes and an escaped rune of n bytes"""
    out = []
    for cp in B_RUNES:
        n = len(utf8(cp))
        for ascii_len in (PATH_CAP - n, PATH_CAP - n + 1):
            for text in (escaped(cp, False), utf8(cp)):
                out.append((b'{"' + b"p" * ascii_len + text + b'":"value"}', ascii_len + n, "p" * ascii_len + chr(cp)))
    return out


# ---- family F: what must be handed back ----
Fault = namedtuple("Fault", "name row handed_back documented_only")


def fault_text(row: bytes) -> bytes:
    """the bytes Go's tokenizer sees for a family F row: raw bytes as they are (an invalid one decodes to U+FFFD there, one byte at a
    time), a lone surrogate escape as U+FFFD"""
    body = row[len(b'{"v":"'):-len(b'"}')]
    if b"\\" not in body:
        return body
    return TR._go_text(json.loads(b'"' + body + b'"')).encode("utf-8")


def fault_rows() -> list:
    out = []

    def add(name, body: bytes, bad: bool, documented_only=False):
        out.append(Fault(name, b'{"v":"a' + body + b'"}', bad, documented_only))

    for name, seq, bad in (("E0 9F", b"\xe0\x9f\x80", True), ("E0 A0", b"\xe0\xa0\x80", False), ("ED 9F", b"\xed\x9f\x80", False), ("ED A0", b"\xed\xa0\x80", True),
                           ("F0 8F", b"\xf0\x8f\x80\x80", True), ("F0 90", b"\xf0\x90\x80\x80", False), ("F4 8F", b"\xf4\x8f\xbf\xbf", False), ("F4 90", b"\xf4\x90\x80\x80", True)):
        add("second byte " + name, seq + b"b", bad)
    for lead in (0xC0, 0xC1, 0xF5, 0xFF):
        add("lead byte %02X" % lead, bytes([lead, 0x80]) + b"b", True)
    add("lead byte C2", b"\xc2\x80b", False)
    add("lead byte F4", b"\xf4\x80\x80\x80b", False)
    add("lone 80", b"\x80b", True)
    add("lone BF", b"\xbfb", True)
    for name, seq in (("C3", b"\xc3"), ("E4", b"\xe4"), ("F0", b"\xf0"), ("E4 B8", b"\xe4\xb8"), ("F0 9F 98", b"\xf0\x9f\x98")):
        add("truncated " + name, seq, True)
    for name, seq in (("C3 A9", b"\xc3\xa9"), ("E4 B8 AD", b"\xe4\xb8\xad"), ("F0 9F 98 80", b"\xf0\x9f\x98\x80")):
        add("complete " + name, seq, False)
    for esc in (b"\\uD800", b"\\uD800A", b"\\uD800\\n", b"\\uD800\\u0041", b"\\uD800\\uD800", b"\\uDC00", b"\\uDFFF"):
        add("surrogate " + esc.decode(), esc, True)
    for esc in (b"\\uD800\\uDC00", b"\\uDBFF\\uDFFF", b"\\udbff\\uDfFf"):
        add("surrogate " + esc.decode(), esc, False)
    add("three hex digits", b"\\u004", True, documented_only=True)             # no valid JSON: handed back or not a row, nothing stronger
    return out
