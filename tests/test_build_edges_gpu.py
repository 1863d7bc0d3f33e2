"""The write side at its edges, bit for bit.  Every case of tests/build_shapes.py goes through bsg_build_hashed under the case's lab
values and must leave exactly the arena its restatement (B.expected_words) names — the whole arena: gap words, a nil filter's place and
the neighbour behind a partial last window included; the output buffer holds 0xA5 bytes beforehand, because the callee zero-fills.  The
cases sit on both sides of the staged / beyond-LDS boundary, of the binned route's window (2^19 bits) and tile (4 096 entries), of the
global-atomic route's slice (8 192 entries) and of for_each_location_x's four-per-trip tail; tests/test_build_shapes.py proves on the CPU
that the table reaches them and that a wrong builder of each kind would be noticed.

Real strings take the same shapes through bsg_build (k_hash_entries on a sub-range of the staging buffer, at a non-zero entry base, for
every binned filter) and through bsg_ingest_build (k_build_sets, and the binning passes over table slots), against the oracle's
build_many; and the mixed call runs once more cut over a context of three entries."""
import numpy as np
import pytest

from bloomsearch_amd._lib import DESC_DTYPE
from bloomsearch_amd.gpu import Context, pack_entries
from oracle import oracle as O
from tests import build_shapes as B
from tests import helpers as H

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
KEY_SHARD_MIN_ENTRIES = 7
W, T, S = B.W, B.T, B.S


class lab:
    """bsg_set_lab keys 6 (bin_min_locs) and 2 (bin_scratch_bytes) for the length of a with-block"""

    def __init__(self, ctx, values):
        self.ctx, self.values = ctx, {**B.LAB_DEFAULTS, **values}

    def __enter__(self):
        for key, value in self.values.items():
            self.ctx.set_lab(key, value)

    def __exit__(self, *exc):
        self.ctx.set_lab(B.KEY_BIN_MIN_LOCS, 4 << 20)
        self.ctx.set_lab(B.KEY_BIN_SCRATCH, 16 << 30)


def desc_array(filters):
    desc = np.zeros(len(filters), dtype=DESC_DTYPE)
    for n, (word_off, m, k) in enumerate(filters):
        desc[n] = (word_off, m, k, 0)
    return desc


def build_hashed(ctx, case, lab_values):
    h, fstart, filters = B.call_arrays(case)
    out = np.full(case.n_words, POISON, dtype=np.uint64)
    with lab(ctx, lab_values):
        got = ctx.build_hashed(h, fstart, desc_array(filters), case.n_words, out=out)
    assert got is out
    return out


# ---- hashed route: the table is the run list ----

@pytest.mark.parametrize("name", list(B.CASES))
def test_hashed_build_leaves_exactly_the_named_bits(ctx, name):
    case = B.CASES[name]
    want = B.expected_words(case)
    got = build_hashed(ctx, case, case.lab)
    assert np.array_equal(got, want), B.difference(case, got, want)
    if case.group in ("window", "tile", "k", "slice"):
        # the same filter under the other beyond-LDS setting (binned <-> global atomics): the two routes against each other
        other = build_hashed(ctx, case, B.other_beyond_lds_lab(case))
        assert np.array_equal(other, got), "under the other beyond-LDS setting, against this one's result: " + B.difference(case, other, got)


# ---- bytes route: real strings, the oracle's build ----

def string_call(name):
    """(entry strings per filter, [(m, k)], layout): the mixed call's geometries, or one filter of n entries at the tile cases' geometry
    behind a small staged one (so that the binned filter's entries start at a non-zero index of the call)"""
    if name.startswith("mixed"):
        shape = B.CASES["mixed-bin-all-tight"]
        return [["f%d-entry-%d" % (n, j) for j in range(len(f.entries))] for n, f in enumerate(shape.filters)], [(f.m, f.k) for f in shape.filters], "tight"
    n = int(name.split("=")[1])
    return [["head-%d" % j for j in range(37)], ["tile-%d-of-%d" % (j, n) for j in range(n)]], [(4099, 7), (B.TILE_M, 10)], "aligned"


STRING_CALLS = {"mixed": (B.BIN_ALL, {B.KEY_BIN_MIN_LOCS: 0, B.KEY_BIN_SCRATCH: B.MIXED_SPLIT_SCRATCH}, {}),
                "tile-n=%d" % T: (B.BIN_ALL,), "tile-n=%d" % (T + 1): (B.BIN_ALL,), "tile-n=%d" % (2 * T + 1): (B.BIN_ALL, B.SLICE_ALL)}


@pytest.mark.parametrize("name", list(STRING_CALLS))
def test_bytes_route_equals_the_oracle(ctx, name):
    strings, geometry, layout = string_call(name)
    filters, n_words = B.lay_out([(m, k, s, None) for (m, k), s in zip(geometry, strings)], layout)
    desc = desc_array([(f.word_off, f.m, f.k) for f in filters])
    blob, off = pack_entries([s for ss in strings for s in ss])
    fstart = np.concatenate([[0], np.cumsum([len(ss) for ss in strings])]).astype(np.uint32)
    want = O.build_many(blob, off, fstart, desc.view(O.DESC_DTYPE), n_words)
    case = B.Case(name, "strings", filters, n_words, {}, layout)
    hashes = ctx.hash_entries(blob, off)
    for values in STRING_CALLS[name]:
        with lab(ctx, values):
            got = ctx.build(blob, off, fstart, desc, n_words, out=np.full(n_words, POISON, dtype=np.uint64))
            hashed = ctx.build_hashed(hashes, fstart, desc, n_words, out=np.full(n_words, POISON, dtype=np.uint64))
        assert np.array_equal(got, want), "bsg_build under %s: %s" % (values, B.difference(case, got, want))
        assert np.array_equal(hashed, want), "bsg_build_hashed(bsg_hash_entries) under %s: %s" % (values, B.difference(case, hashed, want))


# ---- tables route: bsg_ingest_build with caller-chosen geometries ----

# (rows, slots_hint of the token table): its capacity is pow2_at_least(hint) (host/ingest_plan.hpp, layout_tables), and stays that while no table
# grows — the test asserts table_grows == 0 and the table bytes the three capacities come to
TABLE_CLASSES = {"below-one-tile": (100, T // 2), "whole-tiles": (500, 2 * T), "beyond-one-slice": (500, 16 * T)}
TABLE_GEOMETRIES = (B.TABLES_LDS_BITS, B.TABLES_LDS_BITS + 1, 3 * W, 3 * W + 1)
SLOT_BYTES = 40                                                               # host/ingest_plan.hpp kSlotBytes


@pytest.mark.parametrize("table_class", list(TABLE_CLASSES))
def test_tables_route_equals_the_oracle(ctx, table_class):
    """One set of rows, its token filter built at the last staged geometry of this route, one bit beyond it, 3 W and 3 W + 1 — every
    geometry beyond LDS once binned (k_bin_pass over table slots, bin_tile_list) and once with global atomics (k_build_sets' slices)."""
    from oracle import walker_oracle as WO
    n_rows, hint = TABLE_CLASSES[table_class]
    assert hint & (hint - 1) == 0
    assert (hint < T, hint % T == 0 and hint <= 4 * S, hint > 4 * S) == tuple(table_class == c for c in TABLE_CLASSES)
    rows = [('{"msg":"%s","lvl":"L%d"}' % (" ".join("w%dx%d" % (r, j) for j in range(6)), r % 5)).encode() for r in range(n_rows)]
    sets = (set(), set(), set())
    for r in rows:
        WO.index_row(r, sets)
    assert 500 < len(sets[1]) <= hint // 2                                    # a few hundred to a few thousand distinct tokens, at most half the slots
    hints = [256, hint, 1 << 14]
    ing = ctx.ingest_rows(rows, [0, len(rows)], slots_hint=hints, flags=1)
    try:
        assert len(ctx.ingest_fallback_rows(ing)) == 0
        counts, status = ctx.ingest_finish(ing, 1)
        assert [int(x) for x in counts[0]] == [len(s) for s in sets] and not status.any()
        stats = ctx.ingest_stats(ing)
        assert stats.table_grows == 0 and stats.table_bytes == sum(hints) * SLOT_BYTES          # the token table holds `hint` slots
        small = [O.estimate_parameters(len(sets[c]), 0.001) for c in (0, 2)]
        reference = {}
        for m in TABLE_GEOMETRIES:
            staged = B.words_of(m) * 8 + B.K["kSetListBytes"] <= B.K["kLdsBudget"]
            assert staged == (m == B.TABLES_LDS_BITS)
            specs = [(small[0][0], small[0][1], [], None), (m, 10, [], None), (small[1][0], small[1][1], [], None)]
            filters, n_words = B.lay_out(specs, "aligned")
            desc = desc_array([(f.word_off, f.m, f.k) for f in filters])
            if m not in reference:
                want = np.zeros(n_words, dtype=np.uint64)
                for c, f in enumerate(filters):
                    b, o = pack_entries(sorted(sets[c]))
                    d1 = np.zeros(1, dtype=O.DESC_DTYPE)
                    d1[0] = (0, f.m, f.k, 0)
                    want[f.word_off: f.word_off + B.words_of(f.m)] = O.build_many(b, o, np.asarray([0, len(sets[c])], dtype=np.uint32), d1, B.words_of(f.m))
                reference[m] = want
            case = B.Case("%s m=%d" % (table_class, m), "tables", filters, n_words, {}, "aligned")
            for values in ({},) if staged else (B.BIN_ALL, B.SLICE_ALL):
                with lab(ctx, values):
                    got = ctx.ingest_build(ing, desc, n_words, out=np.full(n_words, POISON, dtype=np.uint64))
                assert np.array_equal(got, reference[m]), "under %s: %s" % (values, B.difference(case, got, reference[m]))
    finally:
        ctx.ingest_free(ing)


# ---- parts ----

def test_mixed_call_cut_over_three_entries_gives_the_same_bytes(ctx):
    """bsg_set_lab key 7 = 1: every call with an entry is cut into one part per device, each with its own word range of the caller's
    arena; what no part owns is zeroed by the host."""
    with Context(H.device_ids(3)) as parts:
        parts.set_lab(KEY_SHARD_MIN_ENTRIES, 1)
        for name in ("mixed-bin-all-aligned", "mixed-split-aligned", "mixed-defaults-aligned"):
            case = B.CASES[name]
            before = parts.device_calls().copy()
            got = build_hashed(parts, case, case.lab)
            assert (parts.device_calls() - before).min() >= 1, name          # every entry of the context built a part
            one = build_hashed(ctx, case, case.lab)
            assert np.array_equal(got, one), "three parts against one device: " + B.difference(case, got, one)
            assert np.array_equal(got, B.expected_words(case)), B.difference(case, got, B.expected_words(case))
