"""Per-set MinMax indexes computed by the device ingest (bsg_ingest_rows_minmax / bsg_ingest_open_minmax: k_minmax_rows and
k_minmax_rows_sets, csrc/minmax.hip.h) against the restatement (tests/minmax_restatement.py) over the named shapes and batches of
tests/minmax_shapes.py.

Asserted for every call: the device result with the handed-back rows folded in on the host equals the restatement exactly, per
(set, field), `present` included; the fallback list is ascending, unique and holds every row the shapes name as undecided; counts,
statuses and built filter words equal the same call without fields."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, ingest as I
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.tokenizer import Tokenizer
from tests import minmax_restatement as MR
from tests import minmax_shapes as MS

pytestmark = pytest.mark.gpu

FPR = 0.01
GRAM = Tokenizer(" \t\n\v\f\r", unicode_space=True, lower=True, ngram=3)
VARIANTS = [(0, None), (_lib.INGEST_TRUSTED_JSON, None), (0, GRAM), (_lib.INGEST_TRUSTED_JSON, GRAM)]
VARIANT_IDS = ["validated", "trusted", "validated-3gram", "trusted-3gram"]
BATCHES = MS.batches()


def flatten(row_sets):
    rows = [r for rs in row_sets for r in rs]
    first = np.zeros(len(row_sets) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(rs) for rs in row_sets])
    return rows, first, np.repeat(np.arange(len(row_sets)), np.diff(first.astype(np.int64)))


def as_lists(index, n_fields):
    """(min, max, present) -> per set a list of (min, max) or None, the restatement's form"""
    mn, mx, present = index
    return [[(int(mn[s, f]), int(mx[s, f])) if present[s, f] else None for f in range(n_fields)] for s in range(mn.shape[0])]


def check_fallback(fb, row_sets, first):
    assert list(fb) == sorted(set(int(r) for r in fb)), "the fallback list is not ascending and unique"
    must = {int(first[s]) + i for s, i in MS.undecided_rows(row_sets)}
    assert must <= set(int(r) for r in fb), sorted(must - set(int(r) for r in fb))[:5]


def grouped(ctx, row_sets, fields, flags=0, tokenizer=None, slots_hint=None):
    """one bsg_ingest_rows(_tok | _minmax) call finished and built -> (counts, status, words, fallback rows, raw device index, folded index)"""
    rows, first, set_of_row = flatten(row_sets)
    ing = ctx.ingest_rows(rows, first, None, 0, slots_hint, flags, tokenizer=tokenizer, minmax_fields=fields)
    try:
        fb = ctx.ingest_fallback_rows(ing)
        raw = folded = None
        if fields is not None:
            raw = ctx.ingest_minmax(ing, len(row_sets))
            folded = I.fold_minmax(tuple(a.copy() for a in raw), rows, fb, set_of_row, fields)
        if len(fb):
            entries, sets, kinds = I.host_walk_entries(rows, fb, set_of_row, tokenizer)
            if entries:
                ctx.ingest_add_entries(ing, entries, sets, kinds)
        counts, status = ctx.ingest_finish(ing, len(row_sets))
        if fields is not None:                                       # valid after bsg_ingest_finish too, and unchanged by it
            again = ctx.ingest_minmax(ing, len(row_sets))
            assert all(np.array_equal(a, b) for a, b in zip(raw, again))
        desc, n_words = I.plan_desc(counts, FPR)
        words = ctx.ingest_build(ing, desc, n_words)
        return counts, status, words, fb, raw, folded, ctx.ingest_stats(ing)
    finally:
        ctx.ingest_free(ing)


@pytest.fixture(scope="module")
def plain(ctx):
    """the same calls without fields, once per (batch, variant): counts, statuses and words to compare with"""
    cache = {}

    def get(b, v):
        if (b, v) not in cache:
            flags, tok = VARIANTS[v]
            cache[(b, v)] = grouped(ctx, BATCHES[b][1], None, flags, tok)[:3]
        return cache[(b, v)]
    return get


@pytest.fixture(scope="module")
def want():
    return [MR.set_indexes(row_sets, fields) for _, row_sets, fields in BATCHES]


@pytest.mark.parametrize("v", range(len(VARIANTS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("b", range(len(BATCHES)), ids=[n for n, _, _ in BATCHES])
def test_a_batch_through_the_grouped_call(ctx, plain, want, b, v):
    name, row_sets, fields = BATCHES[b]
    flags, tok = VARIANTS[v]
    counts, status, words, fb, raw, folded, stats = grouped(ctx, row_sets, fields, flags, tok)
    _, first, _ = flatten(row_sets)
    check_fallback(fb, row_sets, first)
    assert stats.n_fallback_rows == len(fb)
    assert as_lists(folded, len(fields)) == want[b]
    p_counts, p_status, p_words = plain(b, v)
    assert np.array_equal(counts, p_counts) and np.array_equal(status, p_status) and np.array_equal(words, p_words)
    assert ctx.last_minmax_ms() > 0
    if name == "a set where every row is handed back":
        assert not raw[2][1].any() and not raw[0][1].any() and not raw[1][1].any()      # the device result of that set is absent
        assert as_lists(folded, len(fields))[1][0] is not None
    if name == "an empty set between two others" or name == "a set without the key":
        assert not raw[2][1].any()


def test_the_scanner_decides_a_row_the_walker_hands_back(ctx):
    """nesting 40 deep is beyond the walker's 16 levels: the walker hands the row back, the scanner's own result holds it already"""
    deep = next(s for s in MS.SHAPES if s.name == "nesting 40 deep")
    _, _, _, fb, raw, folded, _ = grouped(ctx, [[deep.row]], MS.FIELDS)
    assert list(fb) == [0]
    assert as_lists(raw, 3) == [[(11, 11), None, None]] == as_lists(folded, 3)


def test_several_chunks_and_a_table_that_grows(ctx, want):
    """513 rows in chunks of 256, 256 and 1 rows, with token tables of 64 slots: the walk of a chunk re-runs after the tables grew,
    the scanner does not, and the index and the fallback list come out as from one chunk"""
    b = next(i for i, x in enumerate(BATCHES) if x[0] == "one set of 513")
    _, row_sets, fields = BATCHES[b]
    _, first, _ = flatten(row_sets)
    ref = grouped(ctx, row_sets, fields)
    ctx.set_ingest_chunk(1000)
    try:
        counts, status, words, fb, raw, folded, stats = grouped(ctx, row_sets, fields, slots_hint=[64, 64, 64])
    finally:
        ctx.set_ingest_chunk(0)
    assert stats.table_grows > 0
    check_fallback(fb, row_sets, first)
    assert list(fb) == list(ref[3])
    assert as_lists(folded, len(fields)) == want[b] and all(np.array_equal(x, y) for x, y in zip(raw, ref[4]))
    assert np.array_equal(counts, ref[0]) and np.array_equal(status, ref[1]) and np.array_equal(words, ref[2])


def test_malformed_rows_leave_the_other_sets_exact(ctx):
    """truncated rows and rows that are no object sit in a set of their own, whose result is unspecified; the sets beside it are exact
    (validated calls only: BSG_INGEST_TRUSTED_JSON promises the walker valid rows)"""
    row_sets = [MS.size_rows(40), list(MS.MALFORMED) * 5, MS.size_rows(67)[40:]]
    want = MR.set_indexes(row_sets, MS.FIELDS)
    _, _, _, fb, _, folded, _ = grouped(ctx, row_sets, MS.FIELDS)
    got = as_lists(folded, 3)
    assert got[0] == want[0] and got[2] == want[2]
    assert list(fb) == sorted(set(int(r) for r in fb))
    sor = np.repeat(np.arange(3), [len(rs) for rs in row_sets])
    index, _, _, _, _ = stream(ctx, [([r for rs in row_sets for r in rs], sor)], 3, MS.FIELDS)
    got = as_lists(index, 3)
    assert got[0] == want[0] and got[2] == want[2]


# ---- streaming ----
def stream(ctx, batches, n_sets, fields, add_before=None, tokenizer=None, flags=0):
    """batches: [(rows, set_of_row)]; add_before: {batch index: number of sets to add first} -> (folded index, counts, status, words, per-batch fallback lists)"""
    with I.IngestStream.open(ctx, n_sets, None, 0, flags=flags, tokenizer=tokenizer, minmax_fields=fields) as st:
        fbs = []
        for i, (rows, sor) in enumerate(batches):
            if add_before and i in add_before:
                st.add_sets([0xFFFFFFFF] * add_before[i])
            fb = st.append(rows, sor)
            assert list(fb) == sorted(set(int(r) for r in fb))
            fbs.append(fb)
        index = st.minmax()
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        return index, counts, status, st.build(desc, n_words), fbs


@pytest.mark.parametrize("b", [i for i, x in enumerate(BATCHES) if x[0] in ("one set of 513", "every shape its own set", "a set where every row is handed back",
                                                                        "eight fields, hits on the first and the eighth", "an empty set between two others")],
                         ids=lambda i: BATCHES[i][0])
def test_a_stream_in_one_batch_and_in_three_interleaved(ctx, plain, want, b):
    _, row_sets, fields = BATCHES[b]
    rows, first, set_of_row = flatten(row_sets)
    p_counts, p_status, p_words = plain(b, 0)
    # one batch, rows in set order
    index, counts, status, words, fbs = stream(ctx, [(rows, set_of_row)], len(row_sets), fields)
    assert as_lists(index, len(fields)) == want[b]
    check_fallback(fbs[0], row_sets, first)
    assert np.array_equal(counts, p_counts) and np.array_equal(status, p_status) and np.array_equal(words, p_words)
    # the same rows dealt round-robin to three batches, each batch with its sets interleaved
    order = np.argsort(np.arange(len(rows)) * 7919 % 1009, kind="stable")
    cut = [order[k::3] for k in range(3)]
    index, counts, status, words, fbs = stream(ctx, [([rows[i] for i in c], set_of_row[c]) for c in cut], len(row_sets), fields)
    assert as_lists(index, len(fields)) == want[b]
    handed = {int(c[i]) for c, fb in zip(cut, fbs) for i in fb}
    assert {int(first[s]) + i for s, i in MS.undecided_rows(row_sets)} <= handed
    assert np.array_equal(counts, p_counts) and np.array_equal(status, p_status) and np.array_equal(words, p_words)


def test_a_set_added_between_appends_and_small_chunks(ctx):
    """40 sets grow to 90 between two appends (beyond the room the result array was opened with), the second append in chunks of 256
    rows; every set of both generations is exact"""
    first_sets = [MS.size_rows(7 + s)[s:] for s in range(40)]
    more_sets = [MS.size_rows(300 + 3 * s)[295 + s:] for s in range(50)]
    rows1, _, sor1 = flatten(first_sets)
    rows2, _, sor2 = flatten([[]] * 40 + more_sets)
    extra = MS.size_rows(600)                                          # ... and more rows for the first generation, interleaved
    rows2, sor2 = rows2 + extra, np.concatenate([sor2, np.arange(600) % 40])
    ctx.set_ingest_chunk(1000)
    try:
        index, _, status, _, _ = stream(ctx, [(rows1, sor1), (rows2, sor2)], 40, MS.FIELDS, add_before={1: 50})
    finally:
        ctx.set_ingest_chunk(0)
    all_sets = [first_sets[s] + [extra[i] for i in range(s, 600, 40)] for s in range(40)] + more_sets
    assert not status.any() and as_lists(index, 3) == MR.set_indexes(all_sets, MS.FIELDS)


# ---- refusals ----
def test_a_field_less_ingest_has_no_index(ctx):
    ing = ctx.ingest_rows([b'{"ts":1}'], [0, 1])
    try:
        with pytest.raises(BloomGpuError) as e:
            ctx.ingest_minmax(ing, 1)
        assert e.value.code == _lib.BSG_E_INVALID and "without MinMax fields" in str(e.value)
    finally:
        ctx.ingest_free(ing)


@pytest.mark.parametrize("fields,word", [([], "n_fields"), (["f%d" % i for i in range(9)], "n_fields"), (["ts", ""], "field 1"), (["x" * 65], "field 0"),
                                         (["ts", "u", "ts"], "fields 0 and 2")], ids=["none", "nine", "empty", "65 bytes", "equal"])
def test_argument_faults_are_answered_without_a_launch(ctx, fields, word):
    before = ctx.device_calls().copy()
    with pytest.raises(BloomGpuError) as e:
        ctx.ingest_rows([b'{"ts":1}'], [0, 1], minmax_fields=fields)
    assert e.value.code == _lib.BSG_E_INVALID and word in str(e.value)
    with pytest.raises(BloomGpuError) as e:
        ctx.ingest_open(1, minmax_fields=fields)
    assert e.value.code == _lib.BSG_E_INVALID and word in str(e.value)
    assert np.array_equal(ctx.device_calls(), before)


def test_null_field_arrays_are_refused(ctx):
    import ctypes as C
    before = ctx.device_calls().copy()
    out, off, sfr = C.c_uint64(), (C.c_uint64 * 2)(0, 8), (C.c_uint32 * 2)(0, 1)
    row = C.create_string_buffer(b'{"ts":1}', 8)
    fo = (C.c_uint32 * 2)(0, 2)
    assert ctx.L.bsg_ingest_rows_minmax(ctx.h, row, off, 1, sfr, 1, None, 0, None, 0, None, C.byref(out), None, fo, 1) == _lib.BSG_E_INVALID
    assert ctx.L.bsg_ingest_rows_minmax(ctx.h, row, off, 1, sfr, 1, None, 0, None, 0, None, C.byref(out), b"ts", None, 1) == _lib.BSG_E_INVALID
    assert ctx.L.bsg_ingest_open_minmax(ctx.h, 1, None, 0, None, 0, None, C.byref(out), None, None, 1) == _lib.BSG_E_INVALID
    assert np.array_equal(ctx.device_calls(), before)
