"""The write side's build calls at the shapes where its kernels branch: the table of cases tests/test_build_edges_gpu.py runs through
bsg_build_hashed, and a plain restatement of what every call must leave in the caller's arena.  tests/test_build_shapes.py keeps this
file honest (the restated location() against the oracle's, every case's intended route against bsh::build_route, coverage of every
edge computed from the table, and a list of deliberately wrong builders each of which must change some case's expected words).  Test
infrastructure only: no GPU, no call into the library, nothing from the kernels.

What is restated.  bsg_build_hashed takes the four base hashes of every entry; filter f holds entries [fstart[f], fstart[f + 1]) and sets
the bits location(h, i) % m, i < k, with location(h, i) = h[i % 2] + i * h[2 + (((i + i % 2) % 4) / 2)] in wrapping 64-bit arithmetic
(bloom/v3).  The words of filter f start at word_off; every other word of the arena comes back zero.  With h = (h0, h1, 0, 0) every
location is h[i % 2], so an entry NAMES the bit positions p0 = h0 % m and p1 = h1 % m: entry(m, p0, p1) below draws h = p + q m with a
random q, so that the index is a full 64-bit value and not the position itself.

The edges.  W = 2^kBinWindowShift bits is one window of the binned route (k_bin_pass / k_bin_scan / k_bin_apply), T = kBinTile entries
one tile of its passes, S = kBuildSliceEntries entries one slice of the global-atomic route, kLdsBudget * 8 bits the last bitset that
is staged in LDS on the entries route, kBuildThreads the entries one trip of a staged workgroup takes.  All of them are read from the
sources by regex: a changed constant moves the cases with it, a missing one is an error at import.

Unique positions.  Where a lost or doubled entry must show as a specific bit, entry e names the positions (2 e * STEP) % m and
((2 e + 1) * STEP) % m.  STEP is a prime that does not divide m, so a -> (a * STEP) % m is a bijection on [0, m): the 2 n positions of n
entries are pairwise distinct while 2 n <= m, and they spread over every whole window.  unique_entries() asserts both conditions.

Not reachable at test size: binning's limit of n_locs < 2^32 - 4096 (it would take 400 M entries at k = 10), and bitsets of 2^30 bits
and more (tests/test_big_m_gpu.py holds those).  No case here is above 64 W bits; at 64 windows k_bin_scan's running sums stay inside
its first sixteen threads (four windows each), so the scan's carry from one wave to the next is exercised by no case of this table.
"""
from __future__ import annotations

import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
U64 = (1 << 64) - 1


# ---- constants, from the sources ----

def source_constant(rel_path: str, name: str, known: dict) -> int:
    """a `constexpr <type> NAME = <expression>;` of a source file, evaluated over the constants read before it"""
    src = open(os.path.join(CSRC, rel_path)).read()
    found = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
    if not found:
        raise LookupError("%s: no constexpr %s" % (rel_path, name))
    expr = re.sub(r"\b(\d+)(?:ull|ul|u)\b", r"\1", found.group(1), flags=re.I)
    if not re.fullmatch(r"[\w\s*+()<-]+", expr):
        raise LookupError("%s: %s = %s is not plain arithmetic" % (rel_path, name, expr))
    return int(eval(expr, {"__builtins__": {}}, dict(known)))


K = {}
for _path, _name in (("host/build_plan.hpp", "kLdsBudget"), ("host/build_plan.hpp", "kAlignWords"),
                     ("ingest.hip.h", "kBuildSetsThreads"), ("ingest.hip.h", "kSetTile"), ("ingest.hip.h", "kSetListBytes"),
                     ("bin_build.hip.h", "kBinWindowShift"), ("bin_build.hip.h", "kBinMaxWindows"), ("bin_build.hip.h", "kBinThreads"),
                     ("bin_build.hip.h", "kBinTile"), ("kernels.hip.h", "kBuildThreads"), ("bloomgpu.hip", "kBuildSliceEntries")):
    K[_name] = source_constant(_path, _name, K)

LDS_BITS = K["kLdsBudget"] * 8                            # the last bitset staged on the entries route
TABLES_LDS_BITS = (K["kLdsBudget"] - K["kSetListBytes"]) * 8   # ... and on the tables route, beside k_build_sets' list
W = 1 << K["kBinWindowShift"]
T = K["kBinTile"]
S = K["kBuildSliceEntries"]
ALIGN = K["kAlignWords"]
BUILD_THREADS = K["kBuildThreads"]
WORDS_PER_WINDOW = W // 64

KEY_BIN_MIN_LOCS, KEY_BIN_SCRATCH = 6, 2                  # bsg_set_lab keys
LAB_DEFAULTS = {KEY_BIN_MIN_LOCS: 4 << 20, KEY_BIN_SCRATCH: 16 << 30}
STAGED, BINNED, SLICED = "staged", "binned", "sliced"
STEP = 1000003                                            # a prime: see "Unique positions" above
SEED = 20261019


# ---- the restatement ----

def location(h, i: int) -> int:
    """bloom/v3 location(h, i) in Python integers"""
    return (h[i % 2] + i * h[2 + (((i + i % 2) % 4) // 2)]) & U64


def words_of(m: int) -> int:
    return (m + 63) // 64


def windows_of(m: int) -> int:
    return (m + W - 1) // W


# word_off, m, k: the descriptor; entries: [(h0, h1, h2, h3)]; route: the route the filter is meant to take under the case's lab values
# (None for a nil filter)
Filter = namedtuple("Filter", "word_off m k entries route")
# group: window / tile / k / slice / staged / mixed; lab: {key: value} of the bsg_set_lab keys the GPU test applies (a key not named
# keeps its default); layout: aligned / tight / gaps
Case = namedtuple("Case", "name group filters n_words lab layout")


def lab_values(case: Case) -> dict:
    return {**LAB_DEFAULTS, **case.lab}


@functools.lru_cache(maxsize=None)
def _locations(name: str):
    """per filter of case `name`: (entry index, i, location index) of every location, in entry order — three parallel lists"""
    out = []
    for f in CASES[name].filters:
        es, ks, xs = [], [], []
        if f.m:
            for e, h in enumerate(f.entries):
                for i in range(f.k):
                    es.append(e)
                    ks.append(i)
                    xs.append(location(h, i))
        out.append((np.asarray(es, dtype=np.int64), np.asarray(ks, dtype=np.int64), xs))
    return out


class Builder:
    """What a correct build leaves in the arena.  The hooks are where tests/test_build_shapes.py's wrong builders differ."""
    name = "correct"

    def modulus(self, f: Filter) -> int:
        return f.m

    def keep(self, case: Case, f: Filter, e, i, bits):
        """bool per location: is it set?"""
        return np.ones(len(bits), dtype=bool)

    def after(self, case: Case, arena: np.ndarray) -> None:
        pass


def build_words(case: Case, builder: Builder) -> np.ndarray:
    arena = np.zeros(case.n_words, dtype=np.uint64)
    for f, (e, i, xs) in zip(case.filters, _locations(case.name)):
        if f.m == 0 or not xs:
            continue
        mod = builder.modulus(f)
        bits = np.asarray([x % mod for x in xs], dtype=np.int64)
        bits = np.unique(bits[builder.keep(case, f, e, i, bits)])
        bits = bits[bits < words_of(f.m) * 64]             # (a wrong modulus may leave the bitset; the arena's other words are not its to set)
        np.bitwise_or.at(arena, f.word_off + (bits >> 6), np.uint64(1) << (bits & 63).astype(np.uint64))
    builder.after(case, arena)
    return arena


@functools.lru_cache(maxsize=None)
def _expected(name: str) -> np.ndarray:
    words = build_words(CASES[name], Builder())
    words.setflags(write=False)
    return words


def expected_words(case: Case) -> np.ndarray:
    """The whole arena of a case after the call: every named bit set, every other bit — gaps, a nil filter's place, what lies behind a
    partial last window — zero.  Computed once per case and shared read-only."""
    return _expected(case.name)


def span_mask(case: Case) -> np.ndarray:
    """bool per arena word: does it belong to a present filter?"""
    owned = np.zeros(case.n_words, dtype=bool)
    for f in case.filters:
        if f.m:
            assert not owned[f.word_off: f.word_off + words_of(f.m)].any(), case.name
            owned[f.word_off: f.word_off + words_of(f.m)] = True
    return owned


def describe_bit(case: Case, arena_bit: int) -> str:
    """filter, window and position inside the window of one bit of the arena"""
    word = arena_bit >> 6
    for n, f in enumerate(case.filters):
        if f.m and f.word_off <= word < f.word_off + words_of(f.m):
            p = arena_bit - f.word_off * 64
            return "filter %d (m=%d, %s) bit %d = window %d + %d" % (n, f.m, f.route, p, p // W, p % W)
    return "word %d bit %d (no filter's)" % (word, arena_bit & 63)


def difference(case: Case, got: np.ndarray, want: np.ndarray) -> str:
    """the first eight missing and the first eight extra bit positions of an arena that differs"""
    lines = []
    for title, words in (("missing", want & ~got), ("extra", got & ~want)):
        bits = [int(w) * 64 + b for w in np.flatnonzero(words)[:8] for b in range(64) if int(words[w]) >> b & 1][:8]
        lines.append("%s (%d words): %s" % (title, int(np.count_nonzero(words)), "; ".join(describe_bit(case, b) for b in bits) or "none"))
    return "%s: %s" % (case.name, " | ".join(lines))


# ---- entries ----

def entry(rng, m: int, p0: int, p1=None, full=False):
    """an entry that names bit p0 (and p1) of an m-bit filter: h = p + q m with q drawn so that h stays below 2^64.  full: h2 and h3 are
    random, so only location 0 is the named p0 and the others follow the recurrence."""
    def lift(p):
        assert 0 <= p < m
        return p + int(rng.integers(0, (U64 - p) // m, dtype=np.uint64, endpoint=True)) * m
    h0 = lift(p0)
    h1 = lift(p0 if p1 is None else p1)
    if full:
        return (h0, h1) + tuple(int(v) for v in rng.integers(0, U64, size=2, dtype=np.uint64, endpoint=True))
    return (h0, h1, 0, 0)


def pairs(rng, m: int, positions):
    """entries that name the given positions, two per entry (the last one twice where the count is odd)"""
    ps = sorted(set(positions))
    assert all(0 <= p < m for p in ps)
    if len(ps) % 2:
        ps.append(ps[-1])
    return [entry(rng, m, ps[j], ps[j + 1]) for j in range(0, len(ps), 2)]


def unique_positions(m: int, e: int):
    return (2 * e * STEP) % m, ((2 * e + 1) * STEP) % m


def unique_entries(rng, m: int, n: int, full=False):
    """n entries, entry e naming the two positions unique to it (see the module docstring)"""
    assert m % STEP != 0 and STEP % m != 0 and 2 * n <= m
    return [entry(rng, m, *unique_positions(m, e), full=full) for e in range(n)]


def window_positions(m: int, windows=None):
    """every chosen position that fits the geometry: bit 0 and m - 1, the last word's first and last valid bit, and per window (all, or
    the listed ones) its first and last bit and both sides of a u32 and a u64 boundary inside it"""
    ps = {0, m - 1, (words_of(m) - 1) * 64}
    for w in range(windows_of(m)) if windows is None else windows:
        ps |= {w * W + d for d in (0, 31, 32, 63, 64, W - 1)}
    return sorted(p for p in ps if p < m)


# ---- layouts ----

def lay_out(specs, layout: str):
    """specs: [(m, k, entries, route)] -> ([Filter], n_words).  aligned: every filter on a kAlignWords boundary; tight: word_off is the
    running sum of ceil(m / 64), odd offsets included, nothing behind the last filter; gaps: 1 and 17 free words in turn in front of
    every filter (a nil filter's too) and 17 behind the last."""
    filters, at = [], 0
    for n, (m, k, entries, route) in enumerate(specs):
        if layout == "gaps":
            at += (1, 17)[n % 2]
        filters.append(Filter(at, m, k, entries, route if m else None))
        at += words_of(m) if layout != "aligned" else (words_of(m) + ALIGN - 1) // ALIGN * ALIGN
    if layout == "gaps":
        at += 17
    return filters, max(at, 1)


def one_filter(name, group, m, k, entries, route, lab):
    filters, n_words = lay_out([(m, k, entries, route)], "aligned")
    return Case(name, group, filters, n_words, lab, "aligned")


# ---- the table ----

WINDOW_MS = (3 * W, 3 * W + 1, 3 * W + 63, 3 * W + 64, 3 * W + 65, 3 * W - 1, 4 * W - 64, LDS_BITS + 1, 64 * W, 64 * W + 1)
TILE_M = 3 * W + 65
TILE_COUNTS = (1, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T, 2 * T + 1)
TAIL_KS = (1, 2, 3, 4, 5, 8, 9)
SLICE_COUNTS = (S - 1, S, S + 1, 2 * S + 1)
SLICE_MS = (LDS_BITS + 1, 3 * W)
STAGED_MS = (LDS_BITS - 64, LDS_BITS - 63, LDS_BITS)
STAGED_COUNTS = (BUILD_THREADS - 1, BUILD_THREADS, BUILD_THREADS + 1)
RAMP_ZERO_WINDOWS = (3, 8, 9, 10, 11, 37, 63)              # one inside a thread's group of four, one whole group, one alone, the last
BIN_ALL = {KEY_BIN_MIN_LOCS: 0}                           # every bitset beyond LDS that has a location is binned
SLICE_ALL = {KEY_BIN_SCRATCH: 0}                          # none is


def ramp_counts():
    """locations per window of the 64 W case: w + 1, and none in RAMP_ZERO_WINDOWS — pairwise different wherever not zero"""
    return [0 if w in RAMP_ZERO_WINDOWS else w + 1 for w in range(64)]


def _window_cases(rng):
    out = []
    for m in WINDOW_MS:
        out.append(one_filter("window-m=%s" % m_name(m), "window", m, 10, pairs(rng, m, window_positions(m)), BINNED, BIN_ALL))
    m = 3 * W + 65
    out.append(one_filter("window-empty-between", "window", m, 10, pairs(rng, m, window_positions(m, (0, 2, 3)) + [2 * W + 777, 12345]), BINNED, BIN_ALL))
    one = [p for p in window_positions(m, (1,)) if p // W == 1] + [W + 5 * 64 + 7, W + W // 2]
    out.append(one_filter("window-all-in-one", "window", m, 10, pairs(rng, m, one), BINNED, BIN_ALL))
    same = [entry(rng, m, W + 12345) for _ in range(3000)] + pairs(rng, m, [W, 2 * W - 1])
    out.append(one_filter("window-same-bit-3000", "window", m, 10, same, BINNED, BIN_ALL))
    # 64 W: window w holds ramp_counts()[w] locations, one per entry (k = 1): its first bit, its last bit, then distinct random ones
    m, entries = 64 * W, []
    for w, c in enumerate(ramp_counts()):
        inner = rng.choice(W - 2, size=max(c - 2, 0), replace=False) + 1
        for p in ([0, W - 1] + [int(v) for v in inner])[:c]:
            entries.append(entry(rng, m, w * W + p))
    order = rng.permutation(len(entries))                  # the windows' locations arrive interleaved, not window by window
    out.append(one_filter("window-ramp-64W", "window", m, 1, [entries[j] for j in order], BINNED, BIN_ALL))
    return out


def m_name(m: int) -> str:
    for base, label in ((64 * W, "64W"), (4 * W, "4W"), (3 * W, "3W"), (LDS_BITS, "LDS")):
        if abs(m - base) <= 65:
            return label + ("%+d" % (m - base) if m != base else "")
    return str(m)


def _tile_cases(rng):
    out = [one_filter("tile-n=%d" % n, "tile", TILE_M, 10, unique_entries(rng, TILE_M, n), BINNED, BIN_ALL) for n in TILE_COUNTS]
    for k in TAIL_KS:                                      # the four-per-trip tail of for_each_location_x
        out.append(one_filter("tail-k=%d" % k, "k", TILE_M, k, unique_entries(rng, TILE_M, T + 1, full=k > 2), BINNED, BIN_ALL))
    return out


def _slice_cases(rng):
    return [one_filter("slice-m=%s-n=%d" % (m_name(m), n), "slice", m, 10, unique_entries(rng, m, n), SLICED, SLICE_ALL)
            for m in SLICE_MS for n in SLICE_COUNTS]


def _staged_cases(rng):
    out = []
    for lab_name, lab in (("", {}), ("-bin-all", BIN_ALL)):
        for m in STAGED_MS:
            specs = []
            for n in STAGED_COUNTS:                        # three filters of the same geometry, one workgroup each
                edge = pairs(rng, m, [0, m - 1, (words_of(m) - 1) * 64])
                specs.append((m, 10, edge + unique_entries(rng, m, n)[len(edge):], STAGED))
            filters, n_words = lay_out(specs, "aligned")
            out.append(Case("staged-m=%s%s" % (m_name(m), lab_name), "staged", filters, n_words, lab, "aligned"))
    return out


MIXED_BIG_A = (3 * W + 1, 10, 1500)                       # binned; its last window is one word
MIXED_BIG_B = (LDS_BITS + 1, 10, 600)
MIXED_SPLIT_SCRATCH = (4 * MIXED_BIG_A[1] * MIXED_BIG_A[2] + 4 * MIXED_BIG_B[1] * MIXED_BIG_B[2]) // 2     # between the two filters' 4 n k


def _mixed_cases(rng):
    """one call: a staged filter, a nil one, a binned one whose last window is one word, a small staged one directly behind it, a second
    binned one, a filter (beyond LDS) with zero entries"""
    out = []
    for lab_name, lab, big_a, big_b in (("bin-all", BIN_ALL, BINNED, BINNED),
                                        ("split", {KEY_BIN_MIN_LOCS: 0, KEY_BIN_SCRATCH: MIXED_SPLIT_SCRATCH}, SLICED, BINNED),
                                        ("defaults", {}, SLICED, SLICED)):
        for layout in ("aligned", "tight", "gaps"):
            ma, ka, na = MIXED_BIG_A
            mb, kb, nb = MIXED_BIG_B
            ea = pairs(rng, ma, window_positions(ma))
            eb = pairs(rng, mb, window_positions(mb))
            specs = [(100003, 7, pairs(rng, 100003, [0, 100002]) + unique_entries(rng, 100003, 300, full=True), STAGED),
                     (0, 0, [], None),
                     (ma, ka, ea + unique_entries(rng, ma, na)[len(ea):], big_a),
                     (1000, 5, pairs(rng, 1000, [0, 63, 64, 999]) + unique_entries(rng, 1000, 40)[2:], STAGED),
                     (mb, kb, eb + unique_entries(rng, mb, nb)[len(eb):], big_b),
                     (3 * W + 64, 3, [], SLICED)]          # no location: never binned, and the sliced route launches nothing for it
            filters, n_words = lay_out(specs, layout)
            out.append(Case("mixed-%s-%s" % (lab_name, layout), "mixed", filters, n_words, lab, layout))
    return out


def _table():
    rng = np.random.default_rng(SEED)
    cases = _window_cases(rng) + _tile_cases(rng) + _slice_cases(rng) + _staged_cases(rng) + _mixed_cases(rng)
    table = {c.name: c for c in cases}
    assert len(table) == len(cases)
    return table


CASES = _table()


def other_beyond_lds_lab(case: Case) -> dict:
    """the other beyond-LDS setting of a window-, tile-, k- or slice-edge case: binned <-> global atomics"""
    return SLICE_ALL if case.lab == BIN_ALL else BIN_ALL


def call_arrays(case: Case):
    """what bsg_build_hashed takes: (h [n][4] u64, filter_entry_start u32, [(word_off, m, k)])"""
    hs = [h for f in case.filters for h in f.entries]
    h = np.asarray(hs, dtype=np.uint64).reshape(len(hs), 4)
    fstart = np.concatenate([[0], np.cumsum([len(f.entries) for f in case.filters])]).astype(np.uint32)
    return h, fstart, [(f.word_off, f.m, f.k) for f in case.filters]
