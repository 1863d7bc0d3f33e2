"""tests/build_shapes.py is what tests/test_build_edges_gpu.py judges the build kernels with; this file judges it.  The restated
location() is the oracle's; every case's intended route is what bsh::build_route (the code both build paths choose by) answers under the
case's lab values; the edges the table was written for are found in it by computation; and a list of deliberately wrong builders, each
one a way the binned, sliced or staged route could go wrong, changes the expected words of at least one case.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import build_shapes as B
from tests.test_build_plan import driver, run_driver          # noqa: F401  (the build_plan_check fixture, shared by import)

ROUTE_NAMES = {0: B.STAGED, 1: B.BINNED, 2: B.SLICED}
W, T, S = B.W, B.T, B.S


def binned_filters(groups=None):
    return [(c, f) for c in B.CASES.values() if groups is None or c.group in groups for f in c.filters if f.route == B.BINNED]


def named_bits(f):
    """the bit positions a filter's entries name at location 0 and 1"""
    return {h[0] % f.m for h in f.entries} | ({(B.location(h, 1)) % f.m for h in f.entries} if f.k > 1 else set())


def test_constants_are_the_sources():
    assert B.K == {"kLdsBudget": 144 * 1024, "kAlignWords": 16, "kBuildSetsThreads": 1024, "kSetTile": 4096, "kSetListBytes": 16400,
                   "kBinWindowShift": 19, "kBinMaxWindows": 4096, "kBinThreads": 1024, "kBinTile": 4096, "kBuildThreads": 512,
                   "kBuildSliceEntries": 8192}
    assert B.LDS_BITS == 1179648 and B.TABLES_LDS_BITS == 1048448             # the two last staged geometries the issue of this table names
    with pytest.raises(LookupError):
        B.source_constant("bin_build.hip.h", "kNoSuchConstant", {})
    assert all(m < (1 << 30) and B.windows_of(m) <= B.K["kBinMaxWindows"] for c in B.CASES.values() for f in c.filters for m in [f.m])
    assert max(f.m for c in B.CASES.values() for f in c.filters) == 64 * W + 1


def test_restated_location_is_the_oracles():
    rng = np.random.default_rng(5)
    hs = [tuple(int(v) for v in rng.integers(0, B.U64, size=4, dtype=np.uint64, endpoint=True)) for _ in range(300)]
    hs += [(B.U64, B.U64, B.U64, B.U64), (0, 0, 0, 0), (1 << 63, (1 << 63) - 1, 1 << 62, 3), (5, 7, B.U64, 1)]
    hs += [h for name in ("tail-k=9", "window-m=3W+65", "mixed-split-tight") for f in B.CASES[name].filters for h in f.entries[:40]]
    for h in hs:
        for i in range(32):
            assert B.location(h, i) == O.location(h, i), (h, i)
    for h in hs[:50]:
        crafted = (h[0], h[1], 0, 0)
        assert [B.location(crafted, i) for i in range(12)] == [crafted[i % 2] for i in range(12)]


def test_every_crafted_index_is_a_full_width_value():
    """h = p + q m with a random q: the index is not the position"""
    for c in B.CASES.values():
        for f in c.filters:
            if f.entries:
                assert sum(h[0] >= (1 << 40) for h in f.entries) >= 0.9 * len(f.entries) - 1, c.name
                assert all(0 <= v <= B.U64 for h in f.entries for v in h)


def test_intended_routes_are_build_routes(driver, tmp_path):
    rows = [(c, f, len(f.entries), B.lab_values(c)) for c in B.CASES.values() for f in c.filters if f.m]
    ans = run_driver(driver, tmp_path, [[2, f.m, n, f.k, 0, lab[B.KEY_BIN_MIN_LOCS], lab[B.KEY_BIN_SCRATCH]] for _, f, n, lab in rows])
    for c, f, n, _ in rows:
        assert ROUTE_NAMES[ans.take()] == f.route, (c.name, f.m, n, f.k)
    assert ans.done()
    # the beyond-LDS filters of the edge groups flip to the other route under the other setting, as the GPU test relies on
    flips = [(c, f, B.lab_values(c._replace(lab=B.other_beyond_lds_lab(c)))) for c in B.CASES.values() if c.group in ("window", "tile", "k", "slice")
             for f in c.filters]
    ans = run_driver(driver, tmp_path, [[2, f.m, len(f.entries), f.k, 0, lab[B.KEY_BIN_MIN_LOCS], lab[B.KEY_BIN_SCRATCH]] for _, f, lab in flips])
    for c, f, _ in flips:
        assert ROUTE_NAMES[ans.take()] == (B.SLICED if f.route == B.BINNED else B.BINNED), c.name
    assert ans.done()
    assert all(f.route is None for c in B.CASES.values() for f in c.filters if f.m == 0)


def test_layouts_are_what_they_say():
    for c in B.CASES.values():
        owned = B.span_mask(c)                                                # (asserts that no two filters overlap)
        present = [f for f in c.filters if f.m]
        assert all(a.word_off + B.words_of(a.m) <= b.word_off for a, b in zip(present, present[1:])), c.name
        if c.layout == "aligned":
            assert all(f.word_off % B.ALIGN == 0 for f in present), c.name
        if c.layout == "tight":
            assert owned.all() and any(f.word_off % 2 for f in present), c.name
        if c.layout == "gaps":
            gaps = [b.word_off - a.word_off - B.words_of(a.m) for a, b in zip(present, present[1:])]
            assert {1, 17} <= set(gaps) and not owned[-17:].any(), (c.name, gaps)
        assert not B.expected_words(c)[~owned].any(), c.name                    # gap words zero
        for f in present:                                                     # nothing set beyond bit m - 1 of a last word
            if f.m % 64:
                assert int(B.expected_words(c)[f.word_off + B.words_of(f.m) - 1]) >> (f.m % 64) == 0, c.name


def test_mixed_call_is_the_one_described():
    for c in (c for c in B.CASES.values() if c.group == "mixed"):
        f = c.filters
        assert [x.m != 0 for x in f] == [True, False, True, True, True, True] and len(f[5].entries) == 0 and len(f[1].entries) == 0
        assert f[0].route == f[3].route == B.STAGED and f[5].route == B.SLICED and B.words_of(f[5].m) * 8 > B.K["kLdsBudget"]
        assert 0 < f[2].m % W <= 64                                           # its last window is one word
        assert int(B.expected_words(c)[f[3].word_off]) & 1                     # the neighbour's first word is not zero
        if c.layout == "tight":
            assert f[3].word_off == f[2].word_off + B.words_of(f[2].m)        # ... and lies directly behind the partial window
    routes = {c.name.split("-")[1]: (c.filters[2].route, c.filters[4].route) for c in B.CASES.values() if c.group == "mixed"}
    assert routes == {"bin": (B.BINNED, B.BINNED), "split": (B.SLICED, B.BINNED), "defaults": (B.SLICED, B.SLICED)}
    assert {c.layout for c in B.CASES.values() if c.group == "mixed"} == {"aligned", "tight", "gaps"}
    a, b = 4 * B.MIXED_BIG_A[1] * B.MIXED_BIG_A[2], 4 * B.MIXED_BIG_B[1] * B.MIXED_BIG_B[2]
    assert min(a, b) < B.MIXED_SPLIT_SCRATCH < max(a, b)


def test_table_covers_the_edges_it_was_written_for():
    binned = binned_filters()
    assert any(f.m % W == 0 for _, f in binned)
    assert any(0 < f.m % W <= 64 for _, f in binned)
    assert {f.m for c, f in binned if c.group == "window"} >= set(B.WINDOW_MS)
    # an empty interior window between two populated ones
    def populated(f):
        return {p // W for p in named_bits(f)}
    assert any(w - 1 in populated(f) and w + 1 in populated(f) and w not in populated(f) for _, f in binned for w in range(1, B.windows_of(f.m) - 1))
    assert any(len(populated(f)) == 1 and B.windows_of(f.m) > 2 for _, f in binned)                       # all locations in one window
    assert any(max(np.unique([h[0] % f.m for h in f.entries], return_counts=True)[1]) >= 3000 for _, f in binned)   # one bit, 3 000 entries
    # entry counts on both sides of T, 2 T (binned), S (sliced), kBuildThreads (staged)
    n_binned = {len(f.entries) for _, f in binned}
    assert {1, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T, 2 * T + 1} <= n_binned
    sliced = [(c, f) for c in B.CASES.values() for f in c.filters if f.route == B.SLICED]
    assert {(f.m, len(f.entries)) for _, f in sliced} >= {(m, n) for m in (B.LDS_BITS + 1, 3 * W) for n in (S - 1, S, S + 1, 2 * S + 1)}
    staged = [(c, f) for c in B.CASES.values() for f in c.filters if f.route == B.STAGED]
    for m in (B.LDS_BITS - 64, B.LDS_BITS - 63, B.LDS_BITS):
        for lab in ({}, B.BIN_ALL):
            assert {len(f.entries) for c, f in staged if f.m == m and c.lab == lab} >= {B.BUILD_THREADS - 1, B.BUILD_THREADS, B.BUILD_THREADS + 1}, (m, lab)
    assert any(f.m == B.LDS_BITS + 1 for _, f in binned) and any(f.m == B.LDS_BITS + 1 for _, f in sliced)
    assert B.words_of(B.LDS_BITS) * 8 == B.K["kLdsBudget"]                      # the last staged geometry fills all of the dynamic LDS
    for _, f in staged:
        if f.m >= B.LDS_BITS - 64:
            assert {0, f.m - 1, (B.words_of(f.m) - 1) * 64} <= named_bits(f)
    # every k of the list, on the binned route with an entry count that is no multiple of four per thread
    assert {f.k for c, f in binned if c.group == "k" and len(f.entries) == T + 1} == set(B.TAIL_KS) and {f.k for _, f in binned} >= {1, 2, 3, 4, 5, 8, 9, 10}
    assert all(any(h[2] or h[3] for h in f.entries) == (f.k > 2) for c, f in binned if c.group == "k")
    # window-edge cases: for every populated window both its first and its last bit are named where below m (a window that holds a single
    # location, as the 64 W ramp's first, names its first bit), and bit 0, bit m - 1 and the last word's first bit wherever all windows are populated
    for c, f in binned_filters(("window",)):
        bits = named_bits(f)
        per_window = {}
        for h in f.entries:
            for i in range(min(f.k, 2)):
                per_window[B.location(h, i) % f.m // W] = per_window.get(B.location(h, i) % f.m // W, 0) + 1
        for w, n in per_window.items():
            assert w * W in bits, (c.name, w)
            if n > 1 and w * W + W - 1 < f.m:
                assert w * W + W - 1 in bits, (c.name, w)
        if c.name.startswith("window-m="):                                     # every window populated, every chosen position that fits
            assert len(per_window) == B.windows_of(f.m), c.name
            assert {w * W + d for w in range(B.windows_of(f.m)) for d in (0, 31, 32, 63, 64, W - 1) if w * W + d < f.m} <= bits, c.name
            assert {0, f.m - 1, (B.words_of(f.m) - 1) * 64} <= bits, c.name
    # the 64 W ramp: no two populated windows hold the same number of locations, some hold none, and a whole four-window group is empty
    ramp = B.CASES["window-ramp-64W"].filters[0]
    counts = np.bincount([h[0] % ramp.m // W for h in ramp.entries], minlength=64)
    assert counts.tolist() == B.ramp_counts() and len(set(counts[counts > 0].tolist())) == int((counts > 0).sum()) and (counts == 0).sum() >= 3
    assert any(not counts[g * 4: g * 4 + 4].any() for g in range(16)) and any(0 < (counts[g * 4: g * 4 + 4] == 0).sum() < 4 for g in range(16))
    # unique positions: in the tile-, k- and slice-edge cases no two entries share a named position at location 0
    for c in B.CASES.values():
        if c.group in ("tile", "k", "slice"):
            f = c.filters[0]
            assert len({h[0] % f.m for h in f.entries}) == len(f.entries), c.name
            assert len(populated(f)) >= f.m // W or len(f.entries) < 64, c.name       # every whole window takes part


# ---- teeth: wrong builders ----

class DropTileLocal(B.Builder):
    name = "drop the entry at tile-local index T - 1"

    def keep(self, case, f, e, i, bits):
        return e % T != T - 1


class DropTileFirst(B.Builder):
    name = "drop the entry at index T t, t >= 1"

    def keep(self, case, f, e, i, bits):
        return (e % T != 0) | (e == 0)


class LastBitToNextWindow(B.Builder):
    name = "attribute the location w W + W - 1 to window w + 1"

    def keep(self, case, f, e, i, bits):
        return bits % W != W - 1


class ClearWindowFirst(B.Builder):
    name = "clear bit w W, w >= 1"

    def keep(self, case, f, e, i, bits):
        return (bits % W != 0) | (bits == 0)


class ClearLastBit(B.Builder):
    name = "clear bit m - 1"

    def keep(self, case, f, e, i, bits):
        return bits != f.m - 1


class ZeroPartialLastWord(B.Builder):
    name = "zero the last word of a filter whose word count is no multiple of W / 64"

    def after(self, case, arena):
        for f in case.filters:
            if f.m and B.words_of(f.m) % B.WORDS_PER_WINDOW:
                arena[f.word_off + B.words_of(f.m) - 1] = 0


class WriteFullLastWindow(B.Builder):
    name = "write a full last window: zero the first word behind a binned filter's partial window"

    def after(self, case, arena):
        for f in case.filters:
            behind = f.word_off + B.words_of(f.m)
            if f.route == B.BINNED and B.words_of(f.m) % B.WORDS_PER_WINDOW and behind < len(arena):
                arena[behind] = 0


class SkipTail(B.Builder):
    name = "skip the locations i >= 4 floor(k / 4)"

    def keep(self, case, f, e, i, bits):
        return i < f.k // 4 * 4


class ModuloOneMore(B.Builder):
    name = "reduce modulo m + 1"

    def modulus(self, f):
        return f.m + 1


class GapWordLeft(B.Builder):
    name = "leave a gap word non-zero"

    def after(self, case, arena):
        free = np.flatnonzero(~B.span_mask(case))
        if len(free):
            arena[free[0]] = np.uint64(0xA5A5A5A5A5A5A5A5)


class DropSliceFirst(B.Builder):
    name = "drop the entry at index S s, s >= 1"

    def keep(self, case, f, e, i, bits):
        return (e % S != 0) | (e == 0)


class DropTripLast(B.Builder):
    name = "drop the entry at index kBuildThreads of a staged filter"

    def keep(self, case, f, e, i, bits):
        return (e != B.BUILD_THREADS) | (f.route != B.STAGED)


class ClearBitZero(B.Builder):
    name = "clear bit 0"

    def keep(self, case, f, e, i, bits):
        return bits != 0


MUTATIONS = [DropTileLocal(), DropTileFirst(), LastBitToNextWindow(), ClearWindowFirst(), ClearLastBit(), ZeroPartialLastWord(), WriteFullLastWindow(),
             SkipTail(), ModuloOneMore(), GapWordLeft(), DropSliceFirst(), DropTripLast(), ClearBitZero()]


def test_correct_builder_is_the_expectation():
    for c in B.CASES.values():
        assert np.array_equal(B.build_words(c, B.Builder()), B.expected_words(c)) and B.expected_words(c).any(), c.name
        assert not B.expected_words(c).flags.writeable


def test_every_wrong_builder_changes_some_case():
    uncaught, caught_by = [], {}
    for mut in MUTATIONS:
        caught = [c.name for c in B.CASES.values() if not np.array_equal(B.build_words(c, mut), B.expected_words(c))]
        caught_by[mut.name] = caught
        if not caught:
            uncaught.append(mut.name)
    assert not uncaught, "no case of the table notices: %s" % "; ".join(uncaught)
    assert len(MUTATIONS) >= 10
    # the ones that only a particular case can notice are noticed by that case
    assert any(n.startswith("mixed-") and n.endswith("-tight") for n in caught_by[WriteFullLastWindow.name])
    assert any(n.startswith("tile-n=%d" % T) or n.startswith("tile-n=%d" % (2 * T)) for n in caught_by[DropTileLocal.name])
    assert any(n.startswith("slice-") for n in caught_by[DropSliceFirst.name])
    assert any(n.startswith("staged-") for n in caught_by[DropTripLast.name])
    assert {"tail-k=%d" % k for k in (1, 2, 3, 5, 9)} <= set(caught_by[SkipTail.name])


def test_difference_names_filter_window_and_position():
    c = B.CASES["mixed-bin-all-tight"]
    want = B.expected_words(c)
    got = want.copy()
    f = c.filters[2]
    got[f.word_off + (W >> 6)] ^= np.uint64(1)                               # filter 2, window 1, position 0: set or cleared
    got[c.filters[3].word_off] |= np.uint64(1 << 40)
    text = B.difference(c, got, want)
    assert "filter 2" in text and "window 1 + 0" in text and "filter 3" in text and "window 0 + 40" in text, text
