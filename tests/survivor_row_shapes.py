"""Survivor rows (bsg_probe_many_rows) as include/bloomgpu.h describes them, restated in plain Python, and the arenas, query batches and
case lists the GPU edge tests (tests/test_survivor_row_edges_gpu.py) run.  tests/test_survivor_row_shapes.py keeps this file honest: the
crafted arenas have exactly the designed survivors on the oracle, the case list reaches both sides of every tag edge at every row width,
and check_call rejects a list of deliberately wrong encodings.  Test infrastructure only: nothing below comes from gpu.rows_to_dense or
from the kernels.

The contract, from the header.  A row is one (arena, query) pair of a device's shard; it has B blocks (the shard's) and G = ceil(B / 64)
words.  Its tag, in this order: no survivor -> NONE; B survivors -> ALL (this wins over LIST where B <= 2 G); at most 2 G -> LIST;
otherwise DENSE.
  dense layout   header u32 = tag << 30 | survivor count; the payload lies in the row's own slot (words [q G, (q + 1) G) of the arena's
                 rows): a LIST row's `count` ascending u32 ids at the slot's start, a DENSE row's G words; NONE / ALL: slot untouched
  packed layout  header byte = tag << 6 | (count of a LIST row, else 0); the payloads of every run of 256 consecutive queries lie back to
                 back, in query order, from the run's first slot: ceil(count / 2) words for a LIST row, G words for a DENSE row
On a context of nd devices device d holds the blocks d, d + nd, ... of an arena under local numbers (local l = global l nd + d) and
writes into a slice of its own: headers from (d n_arenas) NQ, rows behind the slices of the devices before it.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from bloomsearch_amd import query as Q
from bloomsearch_amd.arena import entry_sets_from_strings, plan_blocks

TAG_NONE, TAG_ALL, TAG_LIST, TAG_DENSE = 0, 1, 2, 3
TAG_NAMES = ("NONE", "ALL", "LIST", "DENSE")
RUN = 256                    # queries whose payloads the packed layout strings together
FPR = 1e-6                   # k = 20: no false positive in any crafted arena (tests/test_survivor_row_shapes.py proves it per size)


def words_of(n_blocks: int) -> int:
    return (n_blocks + 63) // 64


def tag_of(count: int, n_blocks: int) -> int:
    if count == 0:
        return TAG_NONE
    if count == n_blocks:
        return TAG_ALL
    return TAG_LIST if count <= 2 * words_of(n_blocks) else TAG_DENSE


# ---- a. crafted arenas with known survivors ----
# Symbolic counts, ordered so that neighbours in the list carry different tags wherever the arena is large enough to tell them apart
# (DENSE, LIST, NONE, ALL, LIST, DENSE, LIST, DENSE, LIST, DENSE): stretch() puts neighbours on either side of a 256-query boundary.
COUNTS = ("2G+1", "2G", "0", "B", "1", "B-1", "2", "2G+2", "2G-1", "B/2")
PLACES = ("last", "first", "spread")
PATTERNS = [(c, p) for p in PLACES for c in COUNTS]
N_BASE = len(PATTERNS) + 1                     # + one None query: ALL in every arena
ROTATION = 3                                   # query 255 -> pattern 0 (2G+1: DENSE), 256 -> pattern 1 (2G: LIST); 511 -> 1, 512 -> 2 (NONE)


def count_of(sym: str, B: int) -> int:
    G = words_of(B)
    c = {"0": 0, "1": 1, "2": 2, "2G-1": 2 * G - 1, "2G": 2 * G, "2G+1": 2 * G + 1, "2G+2": 2 * G + 2, "B/2": B // 2, "B-1": B - 1, "B": B}[sym]
    return min(max(c, 0), B)


def select(B: int, c: int, place: str) -> np.ndarray:
    """The c blocks of B a pattern selects, ascending."""
    if place == "last":                        # reaches the last valid bit of the last word
        return np.arange(B - c, B, dtype=np.int64)
    if place == "first":
        return np.arange(c, dtype=np.int64)
    return np.arange(c, dtype=np.int64) * B // max(c, 1)      # spread evenly: distinct because c <= B


def design_matrix(B: int) -> np.ndarray:
    """bool [N_BASE][B]: row j = the blocks that hold token s<j>, i.e. the designed survivors of base query j; the last row is the None query."""
    M = np.zeros((N_BASE, B), dtype=bool)
    for j, (sym, place) in enumerate(PATTERNS):
        M[j, select(B, count_of(sym, B), place)] = True
    M[-1] = True
    return M


FILLER = "pad-%d"                              # one more token per block (its own: no two filters alike)


@functools.lru_cache(maxsize=None)
def plan(B: int):
    """The FilterPlan of the crafted arena of B blocks: block b's token filter holds s<j> for every pattern j that selects b, and the filler."""
    M = design_matrix(B)
    blocks = [entry_sets_from_strings([], ["s%d" % j for j in np.flatnonzero(M[:-1, b])] + [FILLER % b], []) for b in range(B)]
    return plan_blocks(blocks, FPR)


BASE_EXPRS = [Q.Token("s%d" % j) for j in range(len(PATTERNS))] + [None]


def stretch(NQ: int) -> np.ndarray:
    """Base query of each of NQ queries: the patterns in cycles, every cycle rotated by ROTATION against the one before."""
    q = np.arange(NQ, dtype=np.int64)
    return (q + ROTATION * (q // N_BASE)) % N_BASE


def exprs_for(NQ: int):
    return [BASE_EXPRS[j] for j in stretch(NQ)]


def bits_to_matrix(words: np.ndarray, B: int) -> np.ndarray:
    """[n][ceil(B / 64)] u64 bitsets (bsg_probe_many's and the oracle's form) -> bool [n][B]."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(len(words), -1)
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not bits[:, B:].any(), "bits at or beyond the block count"
    return bits[:, :B]


# ---- the cases of tests/test_survivor_row_edges_gpu.py ----
WIDTH_BS = [B for G in range(1, 17) for B in (64 * (G - 1) + 1, 64 * G - 1, 64 * G)]      # every staged width: 48 arenas in one call
WIDTH_NQ = 257
QEDGE_BS = (64, 321, 1024)                     # G = 1, 6 (does not divide 256), 16
QEDGE_NQS = (1, 255, 256, 257, 512, 513)
UNSTAGED_BS = (1025, 1088, 1153)               # G = 17, 17, 19: k_survivor_rows' path without the tile
UNSTAGED_NQ = 257
RUN_CYCLE = (1, 65, 130, 64)
RUN_ARENAS = (63, 64, 65, 129)                 # rows_out launches in runs of 64 arenas: one, one, two, three launches
RUN_NQ = 40
SHARD_ND = 3
SHARD_BS = (3 * 1024, 3 * 961)                 # every shard at the packed form's per-device limit / at an odd count below it
SHARD_REFUSED_B = 3 * 1024 + 1                 # device 0 holds 1 025 blocks
SHARD_NQ = 257


def run_blocks(n_arenas: int):
    return [RUN_CYCLE[i % len(RUN_CYCLE)] for i in range(n_arenas)]


def gpu_cases():
    """[(list of block counts, NQ)] of every single-device call the GPU file makes."""
    out = [(list(WIDTH_BS), WIDTH_NQ), (list(UNSTAGED_BS), UNSTAGED_NQ)]
    out += [(list(QEDGE_BS), nq) for nq in QEDGE_NQS]
    out += [(run_blocks(n), RUN_NQ) for n in RUN_ARENAS]
    return out


def all_block_counts():
    return sorted({B for nbs, _ in gpu_cases() for B in nbs} | set(SHARD_BS) | {SHARD_REFUSED_B})


# ---- b. the two layouts ----
Unit = namedtuple("Unit", "d i nl G row_off hdr_at")      # device d's shard of arena i: nl local blocks, first row word, first header


class Layout:
    def __init__(self, nbs, NQ: int, nd: int = 1):
        self.nbs, self.NQ, self.nd = list(nbs), NQ, nd
        self.units = []
        o = 0
        for d in range(nd):
            for i, B in enumerate(self.nbs):
                nl = max(0, (B - d + nd - 1) // nd)
                self.units.append(Unit(d, i, nl, words_of(nl), o, (d * len(self.nbs) + i) * NQ))
                o += NQ * words_of(nl)
        self.row_words = o
        self.hdr_count = nd * len(self.nbs) * NQ           # u32 headers (dense layout) / header bytes (packed layout)


KEEP, SET, ANY = 0, 1, 2          # per byte: not written (still poison) / written with the reference's value / written, value unspecified

Encoded = namedtuple("Encoded", "rows hdr rows_mask hdr_mask layout runs")


def _local(M: np.ndarray, u: Unit, nd: int) -> np.ndarray:
    return M[:, u.d::nd] if nd > 1 else M


def _row_words(bits: np.ndarray, G: int) -> np.ndarray:
    padded = np.zeros(G * 64, dtype=bool)
    padded[: len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


def encode_call(nbs, NQ: int, survivors, packed: bool, poison: int, nd: int = 1, rows_len=None, hdr_len=None) -> Encoded:
    """What a call leaves in two buffers of rows_len u64 / hdr_len u32 pre-filled with the byte `poison`.  survivors[i]: bool [NQ][B_i].
    runs: {(d, i, run)} -> (first word, payload words) of every packed run."""
    L = Layout(nbs, NQ, nd)
    rows = np.full((L.row_words if rows_len is None else rows_len) * 8, poison, dtype=np.uint8)
    hdr = np.full((L.hdr_count if hdr_len is None else hdr_len) * 4, poison, dtype=np.uint8)
    assert len(rows) >= L.row_words * 8 and len(hdr) >= L.hdr_count * 4
    rmask, hmask = np.zeros(len(rows), dtype=np.uint8), np.zeros(len(hdr), dtype=np.uint8)
    hdr32 = hdr.view(np.uint32)
    runs = {}
    for u in L.units:
        M = _local(survivors[u.i], u, nd)
        counts = M.sum(axis=1)
        for q0 in range(0, NQ, RUN):
            cursor = u.row_off + q0 * u.G
            for q in range(q0, min(q0 + RUN, NQ)):
                c = int(counts[q])
                tag = tag_of(c, u.nl)
                if packed:
                    hdr[u.hdr_at + q] = (tag << 6) | (c if tag == TAG_LIST else 0)
                    hmask[u.hdr_at + q] = SET
                    at = cursor
                else:
                    hdr32[u.hdr_at + q] = (tag << 30) | c
                    hmask[(u.hdr_at + q) * 4: (u.hdr_at + q + 1) * 4] = SET
                    at = u.row_off + q * u.G
                if tag == TAG_LIST:
                    rows[at * 8: at * 8 + 4 * c] = np.flatnonzero(M[q]).astype(np.uint32).view(np.uint8)
                    rmask[at * 8: at * 8 + 4 * c] = SET
                    # behind the ids: the odd count's half word (packed), the rest of the slot (dense) — neither is promised by the header
                    rmask[at * 8 + 4 * c: (at + ((c + 1) // 2 if packed else u.G)) * 8] = ANY
                    cursor += (c + 1) // 2
                elif tag == TAG_DENSE:
                    rows[at * 8: (at + u.G) * 8] = _row_words(M[q], u.G).view(np.uint8)
                    rmask[at * 8: (at + u.G) * 8] = SET
                    cursor += u.G
            if packed:
                runs[(u.d, u.i, q0 // RUN)] = (u.row_off + q0 * u.G, cursor - (u.row_off + q0 * u.G))
    return Encoded(rows.view(np.uint64), hdr32, rmask, hmask, L, runs)


def _as_bytes(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _decode_row(tag: int, cnt, payload8: np.ndarray, u: Unit, where) -> np.ndarray:
    """One row's ascending local ids.  cnt: the header's count (None: the packed header of a row that is not a LIST carries none)."""
    if tag == TAG_NONE:
        assert not cnt, ("a NONE row counts survivors", where, cnt)
        return np.zeros(0, dtype=np.int64)
    if tag == TAG_ALL:
        assert cnt is None or cnt == u.nl, ("an ALL row's count is not the block count", where, cnt, u.nl)
        return np.arange(u.nl, dtype=np.int64)
    if tag == TAG_LIST:
        assert 0 < cnt <= 2 * u.G, ("a LIST row's count is outside 1 .. 2 G", where, cnt, u.G)
        ids = payload8[: 4 * cnt].view(np.uint32).astype(np.int64)
        assert (np.diff(ids) > 0).all() and ids[-1] < u.nl, ("a LIST row's ids are not ascending block numbers", where, ids.tolist())
        return ids
    bits = np.unpackbits(payload8[: 8 * u.G], bitorder="little").astype(bool)
    assert not bits[u.nl:].any(), ("a DENSE row sets bits at or beyond the block count", where)
    ids = np.flatnonzero(bits[: u.nl]).astype(np.int64)
    assert cnt is None or cnt == len(ids), ("a DENSE row's count is not the population of its words", where, cnt, len(ids))
    return ids


def decode_call(rows, hdr, nbs, NQ: int, packed: bool, nd: int = 1):
    """-> (ids, tags): ids[i][q] the ascending GLOBAL block ids of (arena i, query q), tags[(d, i)] the NQ tags of a shard.  Raises on
    anything the layouts do not allow (descending ids, ids or bits beyond the block count, counts that disagree with the payload)."""
    L = Layout(nbs, NQ, nd)
    rows8, hdr8 = _as_bytes(rows), _as_bytes(hdr)
    hdr32 = hdr8[: len(hdr8) // 4 * 4].view(np.uint32)
    parts = [[[] for _ in range(NQ)] for _ in L.nbs]
    tags = {}
    for u in L.units:
        t = tags[(u.d, u.i)] = np.zeros(NQ, dtype=np.uint8)
        for q0 in range(0, NQ, RUN):
            cursor = u.row_off + q0 * u.G
            for q in range(q0, min(q0 + RUN, NQ)):
                if packed:
                    h = int(hdr8[u.hdr_at + q])
                    tag, low = h >> 6, h & 63
                    assert tag == TAG_LIST or low == 0, ("a packed header that is not a LIST carries a count", (u.d, u.i, q), h)
                    cnt = low if tag == TAG_LIST else 0 if tag == TAG_NONE else None
                    at = cursor
                else:
                    h = int(hdr32[u.hdr_at + q])
                    tag, cnt = h >> 30, h & 0x3FFFFFFF
                    at = u.row_off + q * u.G
                t[q] = tag
                size = (cnt + 1) // 2 if tag == TAG_LIST else u.G if tag == TAG_DENSE else 0
                assert at + size <= u.row_off + (min(q0 + RUN, NQ) if packed else q + 1) * u.G, ("a payload leaves its slot area", (u.d, u.i, q))
                ids = _decode_row(tag, cnt, rows8[at * 8: (at + size) * 8], u, (u.d, u.i, q))
                cursor += size
                parts[u.i][q].append(ids * nd + u.d)
    ids = [[np.sort(np.concatenate(p)) if p else np.zeros(0, dtype=np.int64) for p in arena] for arena in parts]
    return ids, tags


# ---- c. the one checker of the GPU tests ----
def check_call(rows, hdr, poison: int, nbs, NQ: int, want, packed: bool, nd: int = 1, row_words=None, hdr_words=None):
    """rows / hdr: both buffers WHOLE as a bsg_probe_many_rows call left them, pre-filled with the byte `poison` and longer than the call
    needs; want[i]: bool [NQ][B_i], the oracle's survivors of arena i; row_words / hdr_words: what bsg_survivor_rows_size reported."""
    L = Layout(nbs, NQ, nd)
    if row_words is not None:
        assert (row_words, hdr_words) == (L.row_words, L.hdr_count), ("bsg_survivor_rows_size", row_words, hdr_words, L.row_words, L.hdr_count)
    rows8, hdr8 = _as_bytes(rows), _as_bytes(hdr)
    assert len(rows8) >= L.row_words * 8 and len(hdr8) >= L.hdr_count * 4
    hdr32 = hdr8[: len(hdr8) // 4 * 4].view(np.uint32)
    # 1. every header: the tag rule applied to the oracle's count, and the count the layout asks for
    for u in L.units:
        counts = _local(np.asarray(want[u.i], dtype=bool), u, nd).sum(axis=1)
        for q in range(NQ):
            c = int(counts[q])
            tag = tag_of(c, u.nl)
            if packed:
                h = int(hdr8[u.hdr_at + q])
                got_tag, got_cnt, want_cnt = h >> 6, h & 63, c if tag == TAG_LIST else 0
            else:
                h = int(hdr32[u.hdr_at + q])
                got_tag, got_cnt, want_cnt = h >> 30, h & 0x3FFFFFFF, c
            assert got_tag == tag, "device %d arena %d (%d blocks) query %d: %d survivors are a %s row, the header says %s" % (
                u.d, u.i, u.nl, q, c, TAG_NAMES[tag], TAG_NAMES[got_tag])
            assert got_cnt == want_cnt, "device %d arena %d (%d blocks) query %d: a %s row of %d survivors, the header counts %d" % (
                u.d, u.i, u.nl, q, TAG_NAMES[tag], c, got_cnt)
    # 2. every payload: exactly the oracle's set, ascending
    ids, _ = decode_call(rows8, hdr8, nbs, NQ, packed, nd)
    for i in range(len(L.nbs)):
        for q in range(NQ):
            assert np.array_equal(ids[i][q], np.flatnonzero(want[i][q])), "arena %d query %d: the row's ids are not the oracle's survivors" % (i, q)
    # 3. every byte the call had no business writing still holds the poison: the rows buffer outside the payloads (NONE / ALL slots, a
    #    packed run's area behind its payloads, the tail behind the used part) and the headers behind the last one; every other byte
    #    holds the reference encoding's value, but for those the header leaves open
    ref = encode_call(nbs, NQ, want, packed, poison, nd, len(rows8) // 8, len(hdr8) // 4)
    for name, got, exp, mask in (("rows", rows8, _as_bytes(ref.rows), ref.rows_mask), ("headers", hdr8[: len(ref.hdr) * 4], _as_bytes(ref.hdr), ref.hdr_mask)):
        bad = np.flatnonzero((mask == KEEP) & (got != poison))
        assert len(bad) == 0, "%s: %d bytes outside what the call writes lost the poison, first at byte %d (word %d): %s" % (
            name, len(bad), bad[0], bad[0] // 8, _owner(L, name, int(bad[0]), packed))
        bad = np.flatnonzero((mask == SET) & (got != exp))
        assert len(bad) == 0, "%s: %d written bytes differ from the reference encoding, first at byte %d" % (name, len(bad), bad[0])
    assert (hdr8[len(ref.hdr) * 4:] == poison).all()


def _owner(L: Layout, name: str, byte: int, packed: bool) -> str:
    if name == "rows":
        w = byte // 8
        if w >= L.row_words:
            return "behind the used part (%d words)" % L.row_words
        for u in L.units:
            if u.G and u.row_off <= w < u.row_off + L.NQ * u.G:
                return "device %d arena %d (%d blocks), slot of query %d" % (u.d, u.i, u.nl, (w - u.row_off) // u.G)
    at = byte if packed else byte // 4
    return "behind the last header (%d)" % L.hdr_count if at >= L.hdr_count else "header %d" % at
