"""bsg_match_rows_wide_hist (k_bucket_rows / k_bucket_rows_sets beside the storing walk, k_pair_hist behind k_eval_row_programs): per
(set, query) pair, how many matching rows fall into each bucket of a number field.  The expectation never asks the code under test:
a row's verdict is the restatements' (tests/range_text_cases.verdict, the one the tests of bsg_match_rows_wide_regex_substr_range use),
its slot is tests/hist_restatement.slot_of, and the rows handed back are named by the shapes (an exponent on the field, a backslash in
a top-level key) and by the walker's envelope.  The fallback list must equal the expected list; the expected counts leave out exactly
those rows.  Every call is made with a canary behind the last pair's counters, and every pair's slots must sum to the popcount of the
parent call's bit row minus the handed-back rows that would match."""
import ctypes as C
import functools

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import BSG_E_INVALID, BSG_E_UNSUPPORTED, KIND_FIELD_RANGE, KIND_FIELD_REGEX, KIND_SUBSTRING, KIND_TOKEN, BloomGpuError
from bloomsearch_amd.gpu import Context, wide_pair_bits
from tests import hist_restatement as HR
from tests import hist_shapes as HS
from tests import range_text_cases as RT
from tests import walker_envelope_shapes as WE
from tests.helpers import device_ids
from tests.test_match_wide_range_gpu import RawBatch, csr

pytestmark = pytest.mark.gpu

CANARY = 0xA5C3A5C3
SPEC = ("ts", -40000, 1400, 60)                 # the synthetic rows' ts runs from -50000 to 50002: below, every bucket and above

# (bloom, regex, substring, range): the queries every case draws from, by index
QUERIES = [
    (None, None, None, None),                                                                               # 0 every row
    (Q.FieldToken("level", "error"), None, None, None),                                                     # 1 a third
    (None, None, None, Q.FieldRange("id", 5, 4)),                                                           # 2 no row (lo > hi)
    (None, None, None, Q.FieldRange("id", 10, 40)),                                                         # 3 a range of ids
    (None, None, Q.Substring("in 42 ms"), None),                                                            # 4 sparse
    (None, Q.FieldRegex("level", "^e"), Q.Substring("served in 4"), Q.FieldRange("id", 10, None)),          # 5 all three consumers
    (Q.Token("info"), None, None, None),                                                                    # 6
    (None, None, None, Q.FieldRange("ts", -5, None)),                                                       # 7 a range condition on the bucket field
    (None, Q.FieldRegex("level", "^w"), None, None),                                                        # 8
]


@functools.lru_cache(maxsize=None)
def verdict(q: int, row: bytes) -> bool:
    return RT.verdict(row, *QUERIES[q], None)


def id_is(i):
    """a query that matches exactly the synthetic row i"""
    QUERIES.append((None, None, None, Q.FieldRange("id", i, i)))
    return len(QUERIES) - 1


def call_hist(ctx, rows, batch, spec, first=None, off=None, sq=None, tok=None):
    """the C call with a canary behind the last pair's counters -> (counts [n_pairs, B + 3], fallback rows)"""
    field, origin, width, B = spec
    args, _keep, n, pwo, _total = ctx._wide_args(rows, batch, first, off, sq, tok)
    n_pairs, slots = len(pwo) - 1, _lib.HIST_SLOTS(B)
    counts = np.full(n_pairs * slots + 64, CANARY, dtype=np.uint32)
    fb = np.zeros(max(n, 1), dtype=np.uint32)
    nfb = C.c_uint32()
    name = field.encode()
    ctx._check(ctx.L.bsg_match_rows_wide_hist(*args, name, len(name), origin, width, B, counts.ctypes.data, fb.ctypes.data, len(fb), C.byref(nfb)))
    assert (counts[n_pairs * slots:] == CANARY).all(), "counters were written behind the last pair"
    return counts[: n_pairs * slots].reshape(n_pairs, slots).copy(), fb[: nfb.value].tolist()


def expected(rows, qidx, spec, first, lists, handed_back):
    """-> (counts [n_pairs, B + 3], the fallback list): handed_back names rows by the contract's rules; only those of a set with a
    pair are listed, and exactly those are counted in no slot"""
    B = spec[3]
    listed = sorted(r for s in range(len(lists)) if lists[s] for r in range(int(first[s]), int(first[s + 1])) if r in handed_back)
    counts = np.zeros((sum(len(l) for l in lists), HR.slots(B)), dtype=np.uint32)
    p = 0
    for s, l in enumerate(lists):
        for q in l:
            for r in range(int(first[s]), int(first[s + 1])):
                if r not in handed_back and verdict(qidx[q], rows[r]):
                    counts[p, HR.slot_of(rows[r], *spec)] += 1
            p += 1
    return counts, listed


def check(ctx, rows, qidx, spec, first=None, lists=None, handed_back=(), tok=None):
    """one call against the expectation and against the parent call's bit rows -> (counts, fallback rows)"""
    batch = Q.CompiledWideTextRangeBatch([QUERIES[i] for i in qidx])
    implicit = first is None
    efirst = np.array([0, len(rows)], dtype=np.uint32) if implicit else np.asarray(first, dtype=np.uint32)
    elists = [list(range(len(qidx)))] if implicit else lists
    off, sq = (None, None) if implicit else csr(lists)
    counts, fb = call_hist(ctx, rows, batch, spec, None if implicit else efirst, off, sq, tok)
    want_counts, want_fb = expected(rows, qidx, spec, efirst, elists, set(handed_back))
    assert fb == want_fb
    bad = np.argwhere(counts != want_counts)
    assert not len(bad), (bad[:5].tolist(), [(int(counts[p, s]), int(want_counts[p, s])) for p, s in bad[:5]])
    # each pair's slots sum to the popcount of the parent's bit row, minus the rows handed back beyond the parent's that would match
    words, pwo, pfb = ctx.match_rows_wide_regex_substr_range(rows, batch, None if implicit else efirst, off, sq, tok)
    beyond = sorted(set(fb) - set(pfb.tolist()))
    assert set(pfb.tolist()) <= set(fb)
    p = 0
    for s, l in enumerate(elists):
        lo, hi = int(efirst[s]), int(efirst[s + 1])
        for _ in l:
            bits = wide_pair_bits(words, pwo, p, hi - lo)
            assert int(counts[p].sum()) == int(bits.sum()) - sum(int(bits[r - lo]) for r in beyond if lo <= r < hi), p
            p += 1
    return counts, fb


def walker_hands_back(row: bytes) -> bool:
    """the parent's rules that the shapes meet: the walker's envelope (nesting, path length), and white space other than 0x20 between
    tokens (a JSON string holds no raw tab or line break, so any in the row lies outside one)"""
    return not WE.in_envelope(row) or any(c in row for c in b"\t\n\r")


def synth(n, start=0):
    return [HS.synth_row(start + i) for i in range(n)]


def firsts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


# ---- 1: set sizes at the tile edges, an empty set, a set without a pair, every slot kind ----
SIZES = [1, 63, 64, 65, 129, 0, 4, 5, 70]


def sized_rows(spec):
    """synthetic rows over sets of SIZES rows; the set of 129 rows also holds a row at every edge of the spec's buckets"""
    _, origin, width, B = spec
    rows = synth(sum(SIZES))
    first = firsts(SIZES)
    rows[int(first[6])] = b'{"id":1,"level":"error","ts":1e3}'             # in the set without a pair: never scanned, never handed back
    at = int(first[4])
    rows[at + 3] = b'{"id":20,"level":"error","msg":"no member"}'                            # missing
    rows[at + 64] = b'{"id":21,"level":"error","ts":"17","msg":"a string"}'                  # missing: the last member is no number
    assert origin < -1
    rows[at + 128] = ('{"id":22,"level":"error","ts":1,"ts":%d.5}' % (origin + 1)).encode()  # the last duplicate counts: floor(origin + 1 - 0.5), bucket 0
    for k, t in enumerate((origin - 1, origin, origin + B * width - 1, origin + B * width)):  # below, the first bucket, the last, above
        rows[at + 10 + k] = ('{"id":%d,"level":"error","ts":%d}' % (30 + k, t)).encode()
    return rows, first


@pytest.mark.parametrize("n_buckets", [1, 60, 1024])
def test_sets_at_the_tile_edges_and_every_slot_kind(ctx, n_buckets):
    width = {1: 50000, 60: 1400, 1024: 83}[n_buckets]
    spec = ("ts", -40000, width, n_buckets)
    rows, first = sized_rows(spec)
    last = id_is(int(first[9]) - 1)             # exactly the last row of the last set
    qidx = [0, 1, 2, 3, last]
    # sets of 1, 63, 64, 65 and 129 rows, an empty set with pairs, a set without a pair, a pair that matches no row, one that matches the last row
    lists = [[0], [0, 1], [1], [0, 3], [0, 1, 2], [0, 1], [], [2], [1, 4]]
    counts, fb = check(ctx, rows, qidx, spec, first, lists)
    assert fb == []
    off, _ = csr(lists)
    B = n_buckets
    whole = counts[int(off[4])]                 # query 0 on the set of 129 rows
    assert whole.sum() == 129 and whole[B + 2] == 2 and whole[0] >= 2 and whole[B] >= 1 and whole[B - 1] >= 1 and whole[B + 1] >= 1
    assert counts[int(off[7])].sum() == 0       # the pair that matches no row: zeros, written
    assert counts[int(off[8]) + 1].sum() == 1   # ... and the one that matches exactly the last row of its set


# ---- 2: the shapes over the lanes of two tiles, undecided rows handed back and not counted ----
def test_the_shapes_over_two_tiles(ctx):
    cases = [c for c in HS.CASES if c.name.startswith("shape: ")]
    rows = [c.row for c in cases]
    assert 64 < len(rows) <= 128
    undecided = {i for i, c in enumerate(cases) if c.undecided}
    outside = {i for i, r in enumerate(rows) if walker_hands_back(r)}
    assert len(undecided) >= 9 and len(outside) == 3 and not undecided & outside
    spec = cases[0].spec
    counts, fb = check(ctx, rows, [0, 6], spec, handed_back=undecided | outside)
    assert fb == sorted(undecided | outside)
    # every undecided shape would have matched query 0: none of them is counted
    assert int(counts[0].sum()) == len(rows) - len(fb) and counts[0][HR.missing(60)] > 10
    # ... and the same rows shifted by one lane and split over two sets, the second without a pair
    shifted = synth(1) + rows
    first = np.array([0, 70, len(shifted)], dtype=np.uint32)
    hb = {i + 1 for i in undecided | outside}
    _, fb2 = check(ctx, shifted, [0, 6], spec, first, [[0, 1], []], handed_back=hb)
    assert fb2 == sorted(r for r in hb if r < 70) and len(fb2) < len(hb)


@pytest.mark.parametrize("spec", sorted({c.spec for c in HS.CASES if not c.name.startswith("shape: ")}), ids=lambda s: "%s_%d_%d_%d" % s)
def test_the_bucket_edges(ctx, spec):
    cases = [c for c in HS.CASES if c.spec == spec and not c.name.startswith("shape: ")]
    rows = [c.row for c in cases]
    undecided = {i for i, c in enumerate(cases) if c.undecided}
    counts, fb = check(ctx, rows, [0], spec, handed_back=undecided)
    assert fb == sorted(undecided)
    want = np.zeros(HR.slots(spec[3]), dtype=np.uint32)
    for i, c in enumerate(cases):
        if i not in undecided:
            want[c.want] += 1                   # the slot the case itself names
    assert np.array_equal(counts[0], want)


# ---- 3: one list — the walker's rows and the scanner's ----
def test_a_row_both_hand_back_is_listed_once(ctx):
    rows = synth(70)
    rows[3] = b'{"id":3,"level":"error","ts":2e1,"msg":"x"}'               # the range condition on ts AND the scanner: once
    rows[9] = b'{"id":9,"level":"error","t\\u0073":7,"msg":"x"}'           # the scanner alone (a backslash in a top-level key); it would match query 1
    rows[10] = b'{"id":10,"level":"error","ts":5'                          # the walker alone: a truncated row
    rows[64] = b'{"id":64,"level":"error","other":1e3,"ts":8}'             # an exponent on another key: decided by both
    spec = ("ts", 0, 5, 4)
    # (the truncated row reads as an object with ts 5 to the scanner; what it would say is never counted: the walker hands the row back)
    counts, fb = check(ctx, rows, [7, 1], spec, np.array([0, 70], dtype=np.uint32), [[0, 1]], handed_back={3, 9, 10})
    assert fb == [3, 9, 10]
    assert counts[1][1] >= 1                    # row 64: ts 8 is bucket 1, counted
    # the set that lists only query 1: the exponent on ts is the scanner's alone there
    counts, fb = check(ctx, rows, [7, 1], spec, np.array([0, 70], dtype=np.uint32), [[1]], handed_back={3, 9, 10})
    assert fb == [3, 9, 10]


# ---- 4: a pair over several waves of k_pair_hist (global adds), and more single-wave pairs than one workgroup ----
@pytest.fixture(scope="module")
def big_rows():
    return synth(3000, 100)


@pytest.mark.parametrize("n_buckets", [60, 1024])
def test_a_pair_that_spans_several_waves(ctx, big_rows, n_buckets):
    rows = synth(5) + big_rows + synth(70, 5000)
    first = np.array([0, 5, 3005, 3075], dtype=np.uint32)
    spec = ("ts", -40000, 1400 if n_buckets == 60 else 83, n_buckets)
    counts, fb = check(ctx, rows, [0, 1, 4], spec, first, [[0], [0, 1, 2], [0, 1]])
    assert fb == [] and counts[1].sum() == 3000 and 0 < counts[3].sum() < 100 and counts[2].sum() == 1000 and counts[4].sum() == 70


def test_more_pairs_than_one_workgroup(ctx):
    sizes = [3] * 99 + [7]
    rows = synth(sum(sizes))
    counts, fb = check(ctx, rows, [0, 1, 8], SPEC, firsts(sizes), [[0, 1, 2]] * 100)
    assert counts.shape == (300, 63) and fb == []
    assert counts[0::3].sum() == len(rows)


# ---- 5: the implicit set, and the wrapper ----
def test_the_implicit_set_and_the_python_wrapper(ctx):
    rows = synth(200)
    rows[77] = b'{"id":77,"level":"error","ts":1E2}'
    counts, fb = check(ctx, rows, [0, 1, 2, 5], SPEC, handed_back={77})
    assert fb == [77] and counts[0].sum() == 199 and counts[2].sum() == 0
    batch = Q.CompiledWideTextRangeBatch([QUERIES[i] for i in (0, 1, 2, 5)])
    got, gfb = ctx.match_rows_wide_hist(rows, batch, "ts", SPEC[1], SPEC[2], SPEC[3])
    assert got.shape == (4, 63) and got.dtype == np.uint32 and np.array_equal(got, counts) and gfb.tolist() == [77]
    assert ctx.last_hist_ms() > 0.0 and ctx.last_match_ms() > 0.0
    # the final counts a caller sees: the handed-back row decided on the host
    final = batch.histogram(ctx, rows, "ts", SPEC[1], SPEC[2], SPEC[3])
    extra = np.zeros_like(counts)
    for p, q in enumerate((0, 1, 2, 5)):
        if verdict(q, rows[77]):
            extra[p, HR.slot_of(rows[77], *SPEC)] += 1
    assert extra.sum() == 2 and np.array_equal(final, counts + extra)


# ---- 6: a table from each walker route: the same counts machinery behind each ----
ROUTES = {"plain": ([0, 1, 6], set()), "range_only": ([1, 3, 7], {KIND_FIELD_RANGE}), "substring": ([1, 4, 8], {KIND_SUBSTRING, KIND_FIELD_REGEX}),
          "all_three": ([3, 4, 5], {KIND_FIELD_RANGE, KIND_SUBSTRING, KIND_FIELD_REGEX})}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_walker_route(ctx, route):
    qidx, kinds = ROUTES[route]
    batch = Q.CompiledWideTextRangeBatch([QUERIES[i] for i in qidx])
    assert {k for k in batch.kinds if k > 2} == kinds
    rows = synth(150)
    rows[100] = b'{"id":100,"level":"error","t\\u0073":7,"msg":"request 100 served in 42 ms"}'
    first = np.array([0, 65, 150], dtype=np.uint32)
    counts, fb = check(ctx, rows, qidx, SPEC, first, [[0, 1, 2], [0, 2]], handed_back={100})
    assert fb == [100] and counts.sum() > 0


# ---- 7: rows that travel in several chunks ----
def test_a_set_cut_between_chunks_counts_the_same(ctx):
    rows = [RT.row(id=i, level=("info", "warn", "error")[i % 3], pad="x" * 600, ts=(i * 7919) % 100003 - 50000, msg="request %d served in %d ms" % (i, i % 97))
            for i in range(330)]
    rows[201] = b'{"id":201,"level":"error","ts":17e2,"msg":"x"}'
    assert sum(len(r) for r in rows) > 3 * (1 << 16)             # 64 KiB, the smallest chunk: at least three of them
    first = np.array([0, 110, 220, 330], dtype=np.uint32)
    lists = [[0, 1, 2], [0], [0, 2]]
    one = check(ctx, rows, [0, 1, 4], SPEC, first, lists, handed_back={201})
    try:
        ctx.set_ingest_chunk(1)                                  # its smallest
        many = check(ctx, rows, [0, 1, 4], SPEC, first, lists, handed_back={201})
    finally:
        ctx.set_ingest_chunk(0)
    assert np.array_equal(one[0], many[0]) and one[1] == many[1] == [201] and one[0].sum() > 300


def test_a_set_cut_between_devices_counts_the_same(ctx):
    """two and three aliases of the device, every call cut over them: a set that a part boundary cuts has its counters staged per
    part and added on the host; the counts and the one fallback list are the one-device call's"""
    rows = synth(5) + synth(3000, 100) + synth(70, 5000)
    rows[1500] = b'{"id":1,"level":"error","ts":1e3}'
    rows[3060] = b'{"id":2,"level":"error","t\\u0073":7}'
    first = np.array([0, 5, 3005, 3075], dtype=np.uint32)
    lists = [[0], [0, 1, 2], [0, 1]]
    qidx = [0, 1, 4]
    one = check(ctx, rows, qidx, SPEC, first, lists, handed_back={1500, 3060})
    assert one[1] == [1500, 3060]
    batch = Q.CompiledWideTextRangeBatch([QUERIES[i] for i in qidx])
    off, sq = csr(lists)
    for n_dev in (2, 3):
        with Context(device_ids(n_dev)) as m:
            m.set_lab(7, 1)                                      # every call is cut over the devices, however small
            m.set_lab(8, 1)
            before = m.device_calls()
            counts, fb = call_hist(m, rows, batch, SPEC, first, off, sq)
            assert ((m.device_calls() - before) > 0).sum() == n_dev
            assert np.array_equal(counts, one[0]) and fb == one[1], n_dev
            whole, wfb = call_hist(m, rows, batch, SPEC)         # the implicit set: every part boundary cuts it
            alone, afb = call_hist(ctx, rows, batch, SPEC)
            assert np.array_equal(whole, alone) and wfb == afb == [1500, 3060] and whole[0].sum() == len(rows) - 2
            assert m.last_hist_ms() > 0.0


# ---- 8: refusals before any launch ----
def test_refusals_before_any_launch(ctx):
    rows = synth(10)
    batch = Q.CompiledWideTextRangeBatch([QUERIES[1]])
    before = int(ctx.device_calls().sum())
    for spec, word in [(("ts", 0, 1, 0), "n_buckets"), (("ts", 0, 1, 1025), "n_buckets"), (("ts", 0, 0, 4), "width"), (("", 0, 1, 4), "field_len"),
                       (("y" * 65, 0, 1, 4), "field_len")]:
        with pytest.raises(BloomGpuError) as e:
            call_hist(ctx, rows, batch, spec)
        assert e.value.code == BSG_E_INVALID and word in str(e.value), (spec, str(e.value))
    # null arrays
    args, _keep, n, _pwo, _total = ctx._wide_args(rows, batch, None, None, None, None)
    counts, fb, nfb = np.zeros(64, dtype=np.uint32), np.zeros(16, dtype=np.uint32), C.c_uint32()
    L = ctx.L
    assert L.bsg_match_rows_wide_hist(*args, None, 2, 0, 1, 4, counts.ctypes.data, fb.ctypes.data, 16, C.byref(nfb)) == BSG_E_INVALID
    last_error = lambda: L.bsg_last_error(ctx.h).decode()
    assert "field" in last_error()
    assert L.bsg_match_rows_wide_hist(*args, b"ts", 2, 0, 1, 4, None, fb.ctypes.data, 16, C.byref(nfb)) == BSG_E_INVALID
    assert "out_counts" in last_error()
    assert L.bsg_match_rows_wide_hist(*args, b"ts", 2, 0, 1, 4, counts.ctypes.data, fb.ctypes.data, 16, None) == BSG_E_INVALID
    # what the parent refuses, with the parent's words
    entry = Q.range_entry({"Field": "id", "Lo": 1, "Hi": 2})
    rng, sub = (KIND_FIELD_RANGE, b"id", entry), lambda s: (KIND_SUBSTRING, b"", s)
    for conds, code, words in [([rng] + [sub(b"n%02d" % i) for i in range(64)], BSG_E_UNSUPPORTED, ("65 conditions",)),
                               ([rng, sub(b"abc"), (7, b"m", b"x")], BSG_E_INVALID, ("condition 2", "unknown kind 7")),
                               ([sub(b"abc"), (KIND_FIELD_RANGE, b"id", entry[:16])], BSG_E_INVALID, ("condition 1", "17 bytes")),
                               ([rng, (KIND_FIELD_REGEX, b"m", b"\\bx")], BSG_E_UNSUPPORTED, ("regex condition 1",))]:
        with pytest.raises(BloomGpuError) as e:
            call_hist(ctx, rows, RawBatch(conds), SPEC)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(BloomGpuError) as e:
        call_hist(ctx, rows, RawBatch([rng, sub(b"abc"), (KIND_TOKEN, b"", b"x")], n_queries=3), SPEC, np.array([0, 10], dtype=np.uint32),
                  np.array([0, 3], dtype=np.uint32), np.array([0, 2, 1], dtype=np.uint32))
    assert e.value.code == BSG_E_INVALID and "ascending" in str(e.value)
    assert int(ctx.device_calls().sum()) == before
    # no rows, or no pair: BSG_OK and nothing written
    counts, fb = call_hist(ctx, [], batch, SPEC)
    assert counts.shape == (1, 63) and (counts == CANARY).all() and fb == []
    counts, fb = call_hist(ctx, rows, batch, SPEC, np.array([0, 10], dtype=np.uint32), np.array([0, 0], dtype=np.uint32), np.array([], dtype=np.uint32))
    assert counts.shape == (0, 63) and fb == []
    assert int(ctx.device_calls().sum()) == before
