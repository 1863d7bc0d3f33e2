"""Streaming device ingest (bsg_ingest_open / bsg_ingest_add_sets / bsg_ingest_append_rows: k_ingest_rows_sets over batches whose
rows belong to arbitrary sets in arrival order) against the walker oracle.

Yardstick: oracle/walker_oracle.py's entry sets per set and parent (tests/tokenizer_restatement.py under a tokenizer spec).  A
second witness is the one-shot bsg_ingest_rows(_tok) result over the same rows grouped by set — never the stream itself.
"Equal" means: exact counts, status 0, and bsg_ingest_build_sections bytes identical to the oracle's encoding of its own filters
AND to the one-shot's sections for the same (m, k).
"""
import numpy as np
import pytest

from bloomsearch_amd import _lib, ingest as I, query as Q, synth
from bloomsearch_amd.gpu import Context
from oracle import oracle as O
from oracle import walker_oracle as W
from tests import tokenizer_restatement as R

pytestmark = pytest.mark.gpu

FPR = 0.001
DEEP = b'{"a":' * 18 + b'"too deep"' + b'}' * 18                     # nesting deeper than the device walks (16)
LONE = b'{"s":"\\ud800 lone surrogate"}'                             # a lone surrogate escape: the host walker's


def oracle_sets(rows, spec=None):
    if spec is not None:
        return R.entry_sets(rows, spec)
    sets = (set(), set(), set())
    for r in rows:
        W.index_row(r, sets)
    return sets


def union(triples):
    return tuple(set().union(*(t[k] for t in triples)) for k in range(3))


def group(rows, set_of_row, n_sets):
    out = [[] for _ in range(n_sets)]
    for r, s in zip(rows, set_of_row):
        out[int(s)].append(r)
    return out


def want_sets(row_sets, parent_of_set, n_parents, spec=None, skip=()):
    """the oracle's entry sets in the caller's numbering: sets, then parents"""
    sets = [oracle_sets([r for r in rs if r not in skip], spec) for rs in row_sets]
    return sets + [union([sets[s] for s in range(len(sets)) if parent_of_set[s] == p] or [(set(), set(), set())]) for p in range(n_parents)]


def one_shot_sections(ctx, row_sets, parent_of_set, n_parents, desc, tokenizer=None):
    """the second witness: bsg_ingest_rows(_tok) over the rows grouped by set, built with the same (m, k)"""
    rows = [r for rs in row_sets for r in rs]
    first = np.zeros(len(row_sets) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(rs) for rs in row_sets])
    ing = ctx.ingest_rows(rows, first, parent_of_set if n_parents else None, n_parents, tokenizer=tokenizer)
    try:
        fb = ctx.ingest_fallback_rows(ing)
        if len(fb):
            sor = np.repeat(np.arange(len(row_sets)), np.diff(first.astype(np.int64)))
            entries, sets, kinds = I.host_walk_entries(rows, fb, sor, tokenizer)
            ctx.ingest_add_entries(ing, entries, sets, kinds)
        ctx.ingest_finish(ing, len(row_sets) + n_parents)
        return ctx.ingest_build_sections(ing, desc)
    finally:
        ctx.ingest_free(ing)


def check_counts(counts, status, want, what=""):
    assert not status.any(), (what, status)
    assert [[int(x) for x in c] for c in counts] == [[len(s[k]) for k in range(3)] for s in want], what


def finish_and_check(ctx, st, row_sets, parent_of_set, n_parents, tokenizer=None, what=""):
    want = want_sets(row_sets, parent_of_set, n_parents, tokenizer)
    counts, status = st.finish()
    check_counts(counts, status, want, what)
    desc, _ = I.plan_desc(counts, FPR)
    secs = st.build_sections(desc)
    assert len(secs) == len(want)
    for i, ss in enumerate(want):
        assert secs[i] == O.encode_filter_section([O.build_sized(sorted(ss[k]), FPR) for k in range(3)]), (what, i)
    assert secs == one_shot_sections(ctx, row_sets, parent_of_set, n_parents, desc, tokenizer), what
    return counts, desc, secs


@pytest.fixture(scope="module")
def rows200():
    return synth.rows_json(0, 200)


def test_interleaving_inside_a_wave(ctx, rows200):
    """set_of_row[r] = r % 3: every 64-lane tile of the batch mixes all three sets; one append; nothing handed back"""
    sor = np.arange(200) % 3
    with I.IngestStream.open(ctx, 3, [0, 0, 0], 1) as st:
        fb = st.append(rows200, sor, finish_fallback=False)
        assert len(fb) == 0                      # every row lies inside the device envelope: a run that hands all back must not pass
        stats = st.stats()
        assert stats.n_rows == 200 and stats.n_fallback_rows == 0 and stats.row_bytes == sum(len(r) for r in rows200) and stats.ms_walk > 0
        finish_and_check(ctx, st, group(rows200, sor, 3), [0, 0, 0], 1)


def test_batches_of_uneven_size(ctx, rows200):
    """the same rows in 5 appends of 1, 63, 64, 65 rows and the rest, an empty append in between; batch 3 gives set 1 no row at
    all; set 3 receives its first row only in the last batch; entries repeated across batches are counted once"""
    cuts = [0, 1, 64, 128, 193, 200]
    sor = np.arange(200) % 3
    sor[64:128] = np.arange(64) % 2 * 2          # batch 3: sets 0 and 2 only
    sor[195:] = 3                                # set 3: only in the last batch
    with I.IngestStream.open(ctx, 4, [0, 0, 0, 0], 1) as st:
        for b in range(5):
            lo, hi = cuts[b], cuts[b + 1]
            assert len(st.append(rows200[lo:hi], sor[lo:hi], finish_fallback=False)) == 0
            if b == 2:
                assert len(st.append([], np.zeros(0, np.uint32))) == 0
        assert st.stats().n_rows == 200
        # level / service / words repeat in every batch: the distinct counts are the oracle's over all rows
        finish_and_check(ctx, st, group(rows200, sor, 4), [0, 0, 0, 0], 1)


def test_tables_grow_across_batches():
    """a 64-slot token table receives 40 distinct tokens in batch 1 and 400 more in batch 2: it grows (x4 + rehash from the table,
    not from the rows — batch 1's rows have left the device), and batch 1's entries are still there"""
    def row(i):
        return ('{"m":"%s"}' % " ".join("tok%04d" % (i * 10 + j) for j in range(10))).encode()
    b1 = [row(i) for i in range(4)]
    b2 = [row(i) for i in range(4, 44)]
    filler = synth.rows_json(0, 44)
    hint = np.zeros(6, dtype=np.uint32)
    hint[1] = 64                                 # set 0's token table
    with Context((0,)) as c, I.IngestStream.open(c, 2, [0, 0], 1, slots_hint=hint) as st:
        assert len(st.append(b1 + filler[:4], [0] * 4 + [1] * 4, finish_fallback=False)) == 0
        assert st.stats().table_grows == 0
        rows2 = [x for pair in zip(b2, filler[4:]) for x in pair]            # interleaved
        assert len(st.append(rows2, [0, 1] * 40, finish_fallback=False)) == 0
        assert st.stats().table_grows >= 1
        counts, _, _ = finish_and_check(c, st, [b1 + b2, filler], [0, 0], 1)
        assert int(counts[0, 1]) == 440


def test_add_sets(ctx, rows200):
    """open with 1 set, append; add 2 sets (both to parent 0), append to all three; finish numbers sets 0..2, then the parent"""
    with I.IngestStream.open(ctx, 1, [0], 1) as st:
        assert len(st.append(rows200[:50], [0] * 50)) == 0
        assert st.add_sets([0, 0]) == 1
        sor = np.arange(150) % 3
        assert len(st.append(rows200[50:], sor)) == 0
        g = group(rows200[50:], sor, 3)
        g[0] = rows200[:50] + g[0]
        counts, _, _ = finish_and_check(ctx, st, g, [0, 0, 0], 1)
        assert counts.shape == (4, 3)
    # ... and from no set at all, with more sets than the first descriptor arrays hold (they are regrown, counters kept)
    with I.IngestStream.open(ctx, 0, None, 1) as st:
        assert st.add_sets([0]) == 0
        assert len(st.append(rows200[:20], [0] * 20)) == 0
        assert st.add_sets([0] * 39) == 1
        sor = np.arange(180) % 40
        assert len(st.append(rows200[20:], sor)) == 0
        g = group(rows200[20:], sor, 40)
        g[0] = rows200[:20] + g[0]
        finish_and_check(ctx, st, g, [0] * 40, 1)


def test_fallback_rows_are_returned_by_the_append(ctx):
    rows = synth.rows_json(1000, 70)
    rows[3], rows[68] = DEEP, LONE
    sor = np.arange(70) % 2
    rs = group(rows, sor, 2)
    # before add_entries: the oracle over the other 68 rows — the two rows inserted nothing
    with I.IngestStream.open(ctx, 2, [0, 0], 1) as st:
        fb = st.append(rows, sor, finish_fallback=False)
        assert list(fb) == [3, 68]
        assert st.stats().n_fallback_rows == 2
        counts, status = st.finish()
        check_counts(counts, status, want_sets(rs, [0, 0], 1, skip=(DEEP, LONE)), "without the handed-back rows")
    # after add_entries with the host walker's entries: the full oracle's, the deep row included.  (Only for the lone surrogate the
    # yardstick is the host walker's own sets, as in test_ingest_gpu: it writes U+FFFD, as Go does, where the Python oracle keeps
    # the escape.)
    from tests.test_ingest_gpu import host_sets
    with I.IngestStream.open(ctx, 2, [0, 0], 1) as st:
        assert list(st.append(rows, sor)) == [3, 68]
        counts, status = st.finish()
        want = [union([oracle_sets([r for r in rs[s] if r != LONE]), host_sets([r for r in rs[s] if r == LONE])]) for s in range(2)]
        want.append(union(want))
        assert want[1] != want_sets(rs, [0, 0], 1, skip=(DEEP, LONE))[1]       # (the handed-back rows do add entries)
        check_counts(counts, status, want, "with the host walker's entries")
        desc, _ = I.plan_desc(counts, FPR)
        assert st.build_sections(desc) == one_shot_sections(ctx, rs, [0, 0], 1, desc)
    # room for one index only: the count comes back with BSG_E_INVALID; NULL / 0 only asks for the count
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    off = np.zeros(71, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    s32 = sor.astype(np.uint32)
    with I.IngestStream.open(ctx, 2, [0, 0], 1) as st:
        import ctypes as C
        n, one = C.c_uint32(), np.zeros(1, dtype=np.uint32)
        rc = ctx.L.bsg_ingest_append_rows(ctx.h, st.id, _lib._ptr(blob), _lib._ptr(off), 70, _lib._ptr(s32), _lib._ptr(one), 1, C.byref(n))
        assert rc == _lib.BSG_E_INVALID and n.value == 2 and ctx.L.bsg_last_error(ctx.h)
        n.value = 0
        assert ctx.L.bsg_ingest_append_rows(ctx.h, st.id, _lib._ptr(blob), _lib._ptr(off), 70, _lib._ptr(s32), None, 0, C.byref(n)) == 0
        assert n.value == 2
        # neither call delivered its list: the batch is counted by the call that does, once
        assert st.stats().n_rows == 0 and st.stats().n_fallback_rows == 0
        assert list(st.append(rows, sor)) == [3, 68]
        stats = st.stats()
        assert (stats.n_rows, stats.n_fallback_rows, stats.row_bytes) == (70, 2, int(off[-1]))
    with pytest.raises(TypeError):                                           # the host walker needs the rows as a list
        I.IngestStream(ctx, 0, 2, 1).append((blob, off), sor)


@pytest.mark.parametrize("n_rows", [300, 700])
def test_chunked_upload(n_rows):
    """chunks of the row upload are whole 256-row workgroups (host/row_chunks.hpp), so with a 1 KiB first chunk a 300-row append
    travels in 2 chunks (256 + 44) and a 700-row append in 3 (256 + 256 + 188): each chunk is grouped by set by itself"""
    from tests.test_row_chunks import ingest_plan_before                  # the chunk plan restated in Python
    rows = synth.rows_json(0, n_rows)
    rows[290] = DEEP                             # (in the second chunk: the fallback index must stay batch-local)
    off = [0] + [int(x) for x in np.cumsum([len(r) for r in rows])]
    cuts, _ = ingest_plan_before(off, n_rows, 1024)
    assert len(cuts) - 1 == {300: 2, 700: 3}[n_rows] and cuts[1] == 256, cuts
    sor = (np.arange(n_rows) * 7 + np.arange(n_rows) // 5) % 4
    with Context((0,)) as c:
        try:
            c.set_ingest_chunk(1024)
            with I.IngestStream.open(c, 4, [0, 1, 0, 1], 2) as st:
                assert list(st.append(rows, sor)) == [290]
                finish_and_check(c, st, group(rows, sor, 4), [0, 1, 0, 1], 2)
        finally:
            c.set_ingest_chunk(0)


def test_tokenizer_spec(ctx, rows200):
    from tests.test_tokenizer_ingest_gpu import EDGE_ROWS
    rows = rows200[:90] + EDGE_ROWS
    sor = np.arange(len(rows)) % 3
    spec = R.SPECS["punct_lower"]
    with I.IngestStream.open(ctx, 3, [0, 0, 0], 1, tokenizer=spec) as st:
        st.append(rows, sor)
        finish_and_check(ctx, st, group(rows, sor, 3), [0, 0, 0], 1, tokenizer=spec)
    # a spec equal to the default gives the default's result (and runs the default's kernel)
    from bloomsearch_amd.tokenizer import Tokenizer
    with I.IngestStream.open(ctx, 3, [0, 0, 0], 1, tokenizer=Tokenizer.default()) as st:
        st.append(rows, sor)
        counts, status = st.finish()
        check_counts(counts, status, want_sets(group(rows, sor, 3), [0, 0, 0], 1, Tokenizer.default()))
        desc, _ = I.plan_desc(counts, FPR)
        assert st.build_sections(desc) == one_shot_sections(ctx, group(rows, sor, 3), [0, 0, 0], 1, desc)      # bsg_ingest_rows, no spec


def test_resident_arenas_of_a_streamed_ingest(ctx):
    """bsg_ingest_build_sections with arena ids on a streamed ingest (block i = set i): probing the returned arenas gives the
    tree oracle's verdicts over the oracle's own filters"""
    from bloomsearch_amd.arena import entry_sets_from_strings, plan_blocks
    from tests import helpers as H
    n_sets = 5
    rows = synth.rows_json(0, 400)
    sor = (np.arange(400) * 3) % n_sets
    parents = [0, 0, 0, 1, 1]
    with I.IngestStream.open(ctx, 2, parents[:2], 2) as st:
        st.append(rows[:100], sor[:100] % 2)
        st.add_sets(parents[2:])
        st.append(rows[100:], sor[100:])
        counts, status = st.finish()
        assert not status.any()
        desc, _ = I.plan_desc(counts, FPR)
        secs, a_sets, a_parents = st.build_sections(desc, arenas=True)
    assert a_sets and a_parents
    full_sor = np.concatenate([sor[:100] % 2, sor[100:]])
    want = want_sets(group(rows, full_sor, n_sets), parents, 2)
    d = synth.draws(0, 24)
    exprs = [Q.And(Q.FieldToken("level", synth.LEVELS[d["level"][i]]), Q.FieldToken("user_id", str(int(d["user_id"][i])))) for i in range(24)]
    exprs += [Q.Token("absent-token"), Q.Field("nested.az"), None, Q.Or(Q.Token("nope"), Q.FieldToken("service", synth.SERVICES[0]))]
    cb = Q.compile_queries(exprs)
    ops, poff, _ = cb.arrays()
    bid = ctx.batch_create(H.gpu_terms(ctx, cb), ops, poff)
    try:
        for arena, lo, n in ((a_sets, 0, n_sets), (a_parents, n_sets, 2)):
            plan = plan_blocks([entry_sets_from_strings(*[sorted(s) for s in want[lo + b]]) for b in range(n)], FPR)
            words = O.build_many(plan.blob, plan.off, plan.fstart, plan.desc.view(O.DESC_DTYPE), plan.n_words)
            assert np.array_equal(ctx.probe_batch(arena, bid, cb.n_queries, n), O.survivors_tree(words, plan.desc.view(O.DESC_DTYPE), exprs))
    finally:
        ctx.batch_free(bid)
        ctx.arena_free(a_sets)
        ctx.arena_free(a_parents)


def test_errors_are_reported_before_any_launch(ctx, rows200):
    import ctypes as C
    L, h = ctx.L, ctx.h
    rows = rows200[:4]
    blob = np.frombuffer(b"".join(rows), dtype=np.uint8)
    off = np.zeros(5, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    sor = np.zeros(4, dtype=np.uint32)
    fb, n, out, first = np.zeros(4, dtype=np.uint32), C.c_uint32(), C.c_uint64(), C.c_uint32()
    p = _lib._ptr

    def failed(rc, code):
        assert rc == code, rc
        assert L.bsg_last_error(h), "no message"

    def append(ing, blob_=blob, off_=off, sor_=sor, n_rows=4, fb_=fb, cap=4, n_=n):
        return L.bsg_ingest_append_rows(h, ing, p(blob_), p(off_), n_rows, p(sor_), p(fb_), cap, C.byref(n_) if n_ is not None else None)

    one = np.zeros(1, dtype=np.uint32)
    bad_parent = np.array([0, 1], dtype=np.uint32)
    # open: null id, a parent index >= n_parents, unknown flags, a bad tokenizer
    failed(L.bsg_ingest_open(h, 1, p(one), 1, None, 0, None, None), _lib.BSG_E_INVALID)
    failed(L.bsg_ingest_open(h, 2, p(bad_parent), 1, None, 0, None, C.byref(out)), _lib.BSG_E_INVALID)
    failed(L.bsg_ingest_open(h, 2, None, 1, None, 0, None, C.byref(out)), _lib.BSG_E_INVALID)
    failed(L.bsg_ingest_open(h, 1, p(one), 1, None, 2, None, C.byref(out)), _lib.BSG_E_INVALID)
    failed(L.bsg_ingest_open(None, 1, p(one), 1, None, 0, None, C.byref(out)), _lib.BSG_E_INVALID)
    # unknown ids
    failed(append(0xDEAD), _lib.BSG_E_NOTFOUND)
    failed(L.bsg_ingest_add_sets(h, 0xDEAD, 1, p(one), None, C.byref(first)), _lib.BSG_E_NOTFOUND)
    # an ingest made by bsg_ingest_rows
    shot = ctx.ingest_rows(rows, [0, 4], [0], 1)
    failed(append(shot), _lib.BSG_E_INVALID)
    failed(L.bsg_ingest_add_sets(h, shot, 1, p(one), None, C.byref(first)), _lib.BSG_E_INVALID)
    ctx.ingest_free(shot)
    st = I.IngestStream.open(ctx, 1, [0], 1)
    try:
        failed(append(st.id, sor_=np.array([0, 0, 1, 0], dtype=np.uint32)), _lib.BSG_E_INVALID)       # set >= the current set count
        bad_off = off.copy()
        bad_off[2] = bad_off[1] - 1
        failed(append(st.id, off_=bad_off), _lib.BSG_E_INVALID)                                        # row_off not monotone
        failed(append(st.id, off_=None), _lib.BSG_E_INVALID)
        failed(append(st.id, sor_=None), _lib.BSG_E_INVALID)
        failed(append(st.id, blob_=None), _lib.BSG_E_INVALID)
        failed(append(st.id, n_=None), _lib.BSG_E_INVALID)
        failed(append(st.id, fb_=None, cap=4), _lib.BSG_E_INVALID)
        failed(L.bsg_ingest_add_sets(h, st.id, 2, p(bad_parent), None, C.byref(first)), _lib.BSG_E_INVALID)   # parent >= n_parents
        failed(L.bsg_ingest_add_sets(h, st.id, 1, None, None, C.byref(first)), _lib.BSG_E_INVALID)
        failed(L.bsg_ingest_add_sets(h, st.id, 1, p(one), None, None), _lib.BSG_E_INVALID)
        failed(L.bsg_ingest_fallback_rows(h, st.id, None, 0, C.byref(n)), _lib.BSG_E_INVALID)
        assert b"bsg_ingest_append_rows" in L.bsg_last_error(h)
        assert append(st.id, n_rows=0, off_=None, sor_=None, blob_=None) == _lib.BSG_OK                 # nothing to do, nothing launched
        assert st.stats().n_rows == 0                                                                  # none of the above walked a row
        # ... and the ingest and the context still work
        assert append(st.id) == _lib.BSG_OK and n.value == 0
        counts, status = st.finish()
        check_counts(counts, status, want_sets([rows], [0], 1))
        # already finished
        failed(append(st.id), _lib.BSG_E_INVALID)
        failed(L.bsg_ingest_add_sets(h, st.id, 1, p(one), None, C.byref(first)), _lib.BSG_E_INVALID)
    finally:
        st.close()
    failed(append(st.id if st.id else 0xBEEF), _lib.BSG_E_NOTFOUND)
