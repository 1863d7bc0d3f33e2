"""Shapes of filter sections as k_decode_sections cuts them, restated in plain Python, and the list of section cases the GPU codec tests
(tests/test_section_codec_gpu.py) decode and encode.  tests/test_section_shapes.py keeps the list honest: every class named below has to
stay in it.  Test infrastructure only.

A section is [u8 flags] + per present filter [u32 LE flen = 24 + 8 nw][u64 BE m][u64 BE k][u64 BE m][nw x u64 BE words] + [u32 LE CRC-32C]
(encodeFilterSection, file_format.go:343-384), so its payload is P = 1 + sum(28 + 8 nw) bytes.

The slicing, from the comment of bloomsearch_amd/csrc/crc_slices.h and of k_decode_sections: a section has at most 32 slices (one arrival
flag each); a slice is `unit` bytes, 16 KiB unless 32 of those no longer cover the payload, in which case the unit is the 32nd part of the
payload rounded up to a multiple of 64; slices are counted from the payload's END, slice j = [P - (j + 1) U, P - j U) clipped at 0, so only
the LAST slice (the one that starts at byte 0) is short.  A workgroup checksums its slice in 64-byte granules dealt to 256 threads (G = n //
64 of them, then a tail of n % 64 bytes) and byte-swaps the words that START inside its slice.
"""
from __future__ import annotations

import struct
import zlib
from collections import namedtuple

import numpy as np

from oracle import oracle as O

DEFAULT_UNIT = 16384
MAX_SPLITS = 32
GRANULE = 64


def decode_unit(P: int) -> int:
    per_slice = -(-P // MAX_SPLITS)                   # bytes per slice if the payload went into 32 equal slices
    widened = -(-per_slice // GRANULE) * GRANULE
    return max(DEFAULT_UNIT, widened)


def decode_splits(length: int) -> int:
    """Workgroups a section of `length` bytes (CRC trailer included) takes."""
    if length < 5:
        return 1
    P = length - 4
    return max(1, -(-P // decode_unit(P)))


Shape = namedtuple("Shape", "P U n_split last_slice slices G tail w0 cls straddles")


def payload_size(mask: int, nws) -> int:
    return 1 + sum(28 + 8 * nws[c] for c in range(3) if (mask >> c) & 1)


def classify(mask: int, nws) -> Shape:
    """mask: presence bits (field, token, field-token); nws: words per filter (ignored where absent).
    slices: [(lo, hi)] by slice index j (j = 0 ends at P); G / tail: per slice; w0 / cls: per PRESENT filter, byte offset of its word 0 and
    (P - w0) % 8, which is (lo - w0) % 8 at every slice boundary because the unit is a multiple of 64; straddles: per present filter, whether
    one of its words starts in one slice and ends in the next."""
    P = payload_size(mask, nws)
    U = decode_unit(P)
    n = decode_splits(P + 4)
    slices = [(max(P - (j + 1) * U, 0), P - j * U) for j in range(n)]
    assert slices[-1][0] == 0 and all(hi > lo for lo, hi in slices)
    w0, cls, straddles = {}, {}, {}
    pos = 1
    for c in range(3):
        if not (mask >> c) & 1:
            continue
        w0[c] = pos + 28
        cls[c] = (P - w0[c]) % 8
        end = w0[c] + 8 * nws[c]
        straddles[c] = any(w0[c] < lo < end and (lo - w0[c]) % 8 for lo, _ in slices[:-1])
        pos = end
    assert pos == P
    return Shape(P, U, n, slices[-1][1] - slices[-1][0], slices, [(hi - lo) // GRANULE for lo, hi in slices],
                 [(hi - lo) % GRANULE for lo, hi in slices], w0, cls, straddles)


Case = namedtuple("Case", "name mask nws ms ks")

NA = None          # an absent filter's word count in the case list


def _case(name, mask, nws, exact=(), ks=(3, 7, 5)):
    """m = 64 nw - r with r in 1 .. 63 chosen by the case (bits at and above m are zero in the last word), or exactly 64 nw for the filter kinds
    listed in `exact`."""
    ms = []
    for c in range(3):
        if not (mask >> c) & 1:
            ms.append(0)
            continue
        r = 0 if c in exact else 1 + (len(name) * 7 + nws[c] * 13 + c * 29) % 63
        ms.append(64 * nws[c] - r)
    return Case(name, mask, tuple(nws[c] if (mask >> c) & 1 else 0 for c in range(3)), tuple(ms), ks)


# The smallest shapes that reach each slicing class (tests/test_section_shapes.py names the classes and holds the sizes).  A present filter of
# 0 words is not among them: its m is 0, which the decoder rejects, so there is nothing to decode; it is in header_faults() as a deviation.
# The `plen < 29` branch of the header walk is reached by `flags_only` here and by the short payloads of the header faults.
CASES = [
    _case("flags_only", 0, (NA, NA, NA)),                             # P = 1: all filters nil
    _case("tail_only_1w", 2, (NA, 1, NA)),                            # P = 37: no whole granule
    _case("tail_only_4w", 2, (NA, 4, NA), exact=(1,)),                # P = 61
    _case("one_granule_5w", 2, (NA, 5, NA)),                          # P = 69: G == 1
    _case("largest_single", 2, (NA, 2044, NA)),                       # P = 16 381: 255 granules + tail 61
    _case("flags_byte_slice", 3, (1000, 1041, NA)),                   # P = 16 385: the last slice is the flags byte alone
    _case("last_in_length", 2, (NA, 2045, NA)),                       # P = 16 389: the last slice ends inside the length field
    _case("last_ends_at_w0", 2, (NA, 2048, NA), exact=(1,)),          # P = 16 413: ... exactly at word 0; m = 2^17
    _case("last_word0_only", 2, (NA, 2049, NA)),                      # P = 16 421: ... behind word 0
    _case("two_slices_m5", 5, (1, NA, 2046)),                         # P = 16 433
    _case("three_slices_m3", 3, (2100, 2100, NA)),                    # P = 33 657
    _case("four_slices_m7", 7, (3, 4000, 2500)),                      # P = 52 109
    _case("five_slices", 2, (NA, 10000, NA)),                         # P = 80 029: full middle slices
    _case("thirty_slices_m6", 6, (NA, 30000, 30001), exact=(2,)),     # P = 480 065
    _case("last_default_unit", 2, (NA, 65532, NA)),                   # P = 524 285: 32 slices of 16 384
    _case("first_widened_unit", 2, (NA, 65533, NA)),                  # P = 524 293: 32 slices of 16 448
    _case("one_mib", 2, (NA, 131072, NA), exact=(1,)),                # P = 1 048 605: 32 slices of 32 832; m = 2^23
] + [
    # every presence mask at one three-slice size (4 200 words in all)
    _case("mask%d_three_slices" % mask, mask,
          {1: (4200, NA, NA), 2: (NA, 4200, NA), 4: (NA, NA, 4200), 3: (1300, 2900, NA), 5: (2701, NA, 1499), 6: (NA, 1702, 2498), 7: (1300, 1701, 1199)}[mask])
    for mask in range(1, 8)
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- inputs the GPU tests share: everything below comes from the oracle or from numpy, nothing from the library ----
def dense_filters(case, salt: int = 0):
    """[Filter | None] * 3 with about half the bits below m set and none at or above it; the seed is a function of the case, so no two cases
    (and, with `salt`, no two uses of one case) share words."""
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), salt])
    out = []
    for c in range(3):
        if not (case.mask >> c) & 1:
            out.append(None)
            continue
        w = rng.integers(0, 2 ** 64, size=case.nws[c], dtype=np.uint64)
        if case.ms[c] % 64:
            w[-1] &= np.uint64((1 << (case.ms[c] % 64)) - 1)
        out.append(O.Filter(case.ms[c], case.ks[c], w))
    return out


def arena_of(blocks):
    """blocks: per block [Filter | None] * 3 (or None: a block without filters) -> (words, desc) as the oracle's probe takes them."""
    desc = np.zeros(len(blocks) * 3, dtype=O.DESC_DTYPE)
    parts, cursor = [], 0
    for b, fl in enumerate(blocks):
        for c, f in enumerate(fl or ()):
            if f is None:
                continue
            d = desc[b * 3 + c]
            d["word_off"], d["m"], d["k"] = cursor, f.m, f.k
            parts.append(f.words)
            pad = -len(f.words) % 16
            parts.append(np.zeros(pad, dtype=np.uint64))
            cursor += len(f.words) + pad
    words = np.concatenate(parts) if parts else np.zeros(2, dtype=np.uint64)
    return words, desc


def with_crc(payload: bytes) -> bytes:
    return payload + struct.pack("<I", O.crc32c(payload))


def _filter_bytes(m, k, blen, n_word_bytes, flen=None, fill=0xA5):
    return struct.pack("<I", 24 + n_word_bytes if flen is None else flen) + struct.pack(">QQQ", m, k, blen) + bytes([fill]) * n_word_bytes


def header_faults():
    """Malformed sections, all but the too-short ones under a CORRECT checksum: [(name, section bytes, deviation)].  deviation = the library
    documents that it calls this filter bad where bloom/v3 ReadFrom (the oracle) takes the numbers as they come; for every other entry the
    expected status is the oracle's own code."""
    ok1 = _filter_bytes(64, 3, 64, 8)                    # a good one-word filter: 36 bytes
    out = []
    add = lambda name, sec, dev=False: out.append((name, sec, dev))
    # a flag bit set with fewer than 4 bytes left, at each of the three filter positions
    for left in range(4):
        add("first_header_%d_left" % left, with_crc(bytes([1]) + b"\x20\x00\x00"[:left]))
    add("second_header_2_left", with_crc(bytes([3]) + ok1 + b"\x20\x00"))
    add("third_header_3_left", with_crc(bytes([7]) + ok1 + ok1 + b"\x20\x00\x00"))
    add("third_header_0_left_mask5", with_crc(bytes([5]) + ok1))
    # a length one more than what is left
    add("flen_one_too_long", with_crc(bytes([2]) + _filter_bytes(64, 3, 64, 8, flen=33)))
    # lengths around the 24 header bytes, each followed by exactly that many bytes
    for flen in (23, 24, 25):
        add("flen_%d" % flen, with_crc(bytes([1]) + (_filter_bytes(64, 3, 64, 8, flen=flen))[: 4 + flen]))
    # a second and a third header with 4, 27 and 28 bytes left: the length alone, the last non-batched read, the first batched one
    for left in (4, 27, 28):
        add("second_header_%d_left" % left, with_crc(bytes([3]) + ok1 + ok1[:left]))
        add("third_header_%d_left" % left, with_crc(bytes([7]) + ok1 + ok1 + ok1[:left]))
    add("second_header_28_left_flen_24", with_crc(bytes([6]) + ok1 + _filter_bytes(64, 3, 64, 0)))
    # the bitset needs one word more than the length holds
    add("bitset_one_word_short", with_crc(bytes([2]) + _filter_bytes(128, 3, 129, 16)))
    # trailing bytes
    add("trailing_1", with_crc(bytes([1]) + ok1 + b"\x00"))
    add("trailing_8", with_crc(bytes([4]) + ok1 + b"\x00" * 8))
    # unknown flag bits
    add("flag_0x08", with_crc(bytes([1 | 0x08]) + ok1))
    add("flag_0x80", with_crc(bytes([2 | 0x80]) + ok1))
    # too small to hold a checksum and a flags byte
    for n in range(1, 5):
        add("len_%d" % n, bytes([1, 2, 3, 4][:n]))
    # the truncation again in a section of three slices: every slice's own header walk meets it
    big = bytes([3]) + _filter_bytes(64 * 2100, 3, 64 * 2100, 8 * 2100) + _filter_bytes(64 * 2100, 3, 64 * 2100, 8 * 2099, flen=24 + 8 * 2100)
    assert decode_splits(len(big) + 4) == 3
    add("truncated_three_slices", with_crc(big))
    add("third_header_2_left_three_slices", with_crc(bytes([7]) + _filter_bytes(64 * 2100, 3, 64 * 2100, 8 * 2100) * 2 + b"\x20\x00"))
    # deviations: bloom/v3 ReadFrom (the oracle) takes m, k and the bitset length as they come and ACCEPTS each of these sections; the decoder
    # answers "bad filter".  include/bloomgpu.h documents a bitset shorter than m and k beyond 1 024; an m whose (m + 63) / 64 wraps is the
    # same check.  m = 0 (a header with 0 words) and k = 0 are rejected too (parse_section_header: `mm == 0 || kk == 0`) although the header
    # does not list them: a filter with m = 0 divides by zero at its first probe and one with k = 0 matches everything.
    add("bitset_shorter_than_m", with_crc(bytes([1]) + _filter_bytes(65, 3, 64, 8)), True)
    add("k_1025", with_crc(bytes([1]) + _filter_bytes(64, 1025, 64, 8)), True)
    add("m_wraps", with_crc(bytes([1]) + _filter_bytes(2 ** 64 - 1, 3, 64, 8)), True)
    add("m_0_no_words", with_crc(bytes([1]) + _filter_bytes(0, 3, 0, 0)), True)
    add("k_0", with_crc(bytes([1]) + _filter_bytes(64, 0, 64, 8)), True)
    return out


def oracle_code(section: bytes) -> int:
    """0, or parseFilterSection's error code as the oracle reports it (the C function's own return value: nothing is decoded)."""
    if not section:
        return 0
    import ctypes as C
    buf = np.frombuffer(section, dtype=np.uint8)
    present, m, k, woff = (C.c_int * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    return int(O.lib().bo_parse_filter_section(buf.ctypes.data, len(section), present, m, k, woff))


VOCAB = ["tok%d" % i for i in range(4000)] + ["Ünï%d" % i for i in range(40)]


def entry_plan(specs, seed: int, n_tokens: int = 40):
    """specs: per block a Case (its mask, ms, ks are taken) or None (a block without a section).  -> blob, off, fstart, desc, n_words for
    bsg_build / the oracle's build, and per block its (fields, tokens, [(field, token)]) strings."""
    rng = np.random.default_rng(seed)
    desc = np.zeros(len(specs) * 3, dtype=O.DESC_DTYPE)
    entries, fstart, strings, cursor = [], [0], [], 0
    for b, case in enumerate(specs):
        fields = ["f%d" % i for i in rng.choice(40, size=5, replace=False)]
        toks = sorted({VOCAB[i] for i in rng.integers(0, len(VOCAB), size=n_tokens)})
        pairs = sorted({(fields[int(rng.integers(0, len(fields)))], t) for t in toks})
        sets = (fields, toks, [f + "::" + t for f, t in pairs])
        kept = [[], [], []]
        for c in range(3):
            if case is not None and (case.mask >> c) & 1:
                d = desc[b * 3 + c]
                d["word_off"], d["m"], d["k"] = cursor, case.ms[c], case.ks[c]
                cursor += (case.nws[c] + 15) // 16 * 16
                entries += [s.encode() for s in sets[c]]
                kept[c] = sets[c] if c < 2 else pairs
            fstart.append(len(entries))
        strings.append(tuple(kept))
    blob, off = O.pack_entries(entries)
    return blob, off, np.asarray(fstart, dtype=np.uint32), desc, max(cursor, 2), strings


def sections_from_words(specs, words, desc):
    """The oracle's encoding of every block (b"" where the spec is None; a 5-byte all-nil section where its mask is 0)."""
    out = []
    for b, case in enumerate(specs):
        out.append(b"" if case is None else O.encode_filter_section(O.block_filters(words, desc, b)))
    return out
