"""The keyed streaming ingest (bsg_ingest_open_keyed / _append_rows_keyed / _add_sets_keyed / _keys: k_partition_rows and
k_partition_assign in front of the walkers) against the restatement of its rule (tests/partition_restatement.py).

Yardsticks, never the keyed route itself: every row's set, the hand-backs and the key -> set map come from the restatement; counts,
statuses, filter words and MinMax indexes come from an ingest fed through bsg_ingest_append_rows with the restatement's sets.  Every
comparison is exact."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, ingest as I, synth
from bloomsearch_amd._lib import BloomGpuError
from tests import ngram_restatement as G
from tests import partition_restatement as PR
from tests import partition_shapes as PS
from tests import tokenizer_restatement as R

pytestmark = pytest.mark.gpu

FPR = 0.001
UND = _lib.SET_UNDECIDED
TOKS = {"default": None, "punct_lower": R.SPECS["punct_lower"], "tri_default": G.SPECS["tri_default"]}
TOK_IDS = list(TOKS)


def tenant_rows(first, n, key_of):
    """synth rows with a partition member in front: key_of(i) gives row i's value as JSON text"""
    return [b'{"tenant":' + key_of(first + i).encode() + b"," + r[1:] for i, r in enumerate(synth.rows_json(first, n))]


def plain_route(ctx, batches, sets, tok, minmax_fields=None, n_sets=0, finish_fallback=True):
    """the reference: bsg_ingest_append_rows with the given sets (None: the row is left out), at least n_sets sets;
    -> counts, status, words, minmax"""
    with I.IngestStream.open(ctx, 0, None, 1, tokenizer=tok, minmax_fields=minmax_fields) as st:
        for rows, ss in zip(batches, sets):
            top = max([s for s in ss if s is not None] + [n_sets - 1]) + 1
            if top > st.n_sets:
                st.add_sets([0] * (top - st.n_sets))
            keep = [i for i, s in enumerate(ss) if s is not None]
            st.append([rows[i] for i in keep], [ss[i] for i in keep], finish_fallback=finish_fallback)
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        return counts, status, st.build(desc, n_words), (st.minmax() if minmax_fields else None)


def finish_on_host(ctx, st, rows, sets, fb, name):
    """what a caller does with a keyed batch's hand-backs: the undecided rows' texts (here: the restatement's) are registered, then
    every handed-back row is walked by the host walker"""
    und = [int(r) for r in fb if sets[int(r)] == UND]
    if und:
        sets[und] = st.add_keys([PR.partition_text(rows[r], name) for r in und])
    if len(fb):
        entries, esets, kinds = I.host_walk_entries(rows, fb, sets, st.tokenizer)
        if entries:
            ctx.ingest_add_entries(st.id, entries, esets, kinds)


def keyed_route(ctx, batches, name, tok, known=None):
    """the keyed stream over the batches, every append checked against the restatement and its hand-backs finished on the host;
    -> counts, status, words, keys"""
    keys = list(known or [])
    with I.IngestStream.open(ctx, 0, 0, 1, tokenizer=tok, partition_field=name) as st:
        if keys:
            assert list(st.add_keys(keys)) == list(range(len(keys)))
        for b, rows in enumerate(batches):
            sets, fb = st.append_keyed(rows, finish_fallback=False)
            raw, raw_keys = PR.assign_sets([rows], name, known=keys)
            assert [None if s == UND else int(s) for s in sets] == raw[0], ("batch", b)
            assert st.keys() == raw_keys and st.n_sets == len(raw_keys)
            undecided = [i for i, s in enumerate(raw[0]) if s is None]
            assert set(undecided) <= set(int(r) for r in fb) and list(fb) == sorted(set(int(r) for r in fb))
            finish_on_host(ctx, st, rows, sets, fb, name)
            full, keys = PR.assign_sets([rows], name, known=keys, host_finish=True)
            assert [int(s) for s in sets] == full[0] and st.keys() == keys
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        return counts, status, st.build(desc, n_words), st.keys()


def same(a, b, what=""):
    assert np.array_equal(a[0], b[0]), (what, "counts")
    assert np.array_equal(a[1], b[1]) and not a[1].any(), (what, "status")
    assert np.array_equal(a[2], b[2]), (what, "filter words")


@pytest.mark.parametrize("tok", TOK_IDS)
def test_batches_at_the_lane_wave_and_workgroup_edges(ctx, tok):
    """appends of 1, 63, 64, 65 and 257 rows; five texts ("5" and 5 are one), a text first met in each batch, rows without the member"""
    vals = ['"a"', '"b"', '5', '"5"', 'true', '"late"', 'null', '1.0']
    cuts = [0, 1, 64, 128, 193, 450]
    rows = tenant_rows(0, 450, lambda i: vals[(i * 7 + i // 64) % (3 + i // 90)])
    rows[100] = b"{" + rows[100][rows[100].index(b",") + 1:]                                  # no member: the empty text
    batches = [rows[cuts[i]: cuts[i + 1]] for i in range(5)]
    got = keyed_route(ctx, batches, "tenant", TOKS[tok])
    sets, keys = PR.assign_sets(batches, "tenant", host_finish=True)
    assert got[3] == keys and b"5" in keys and keys.count(b"5") == 1
    same(got, plain_route(ctx, batches, sets, TOKS[tok]), tok)


@pytest.mark.parametrize("tok", TOK_IDS)
def test_the_shapes_in_one_batch(ctx, tok):
    """every shape at every alignment: the undecided rows are exactly the predicted ones, carry BSG_SET_UNDECIDED, are in the list and
    have inserted nothing; once finished on the host the filters equal the route with explicit sets"""
    for field in ("p", "ts", PS.NAME64):
        shapes = [s for s in PS.SHAPES if s.field == field]
        pairs = PS.at_every_alignment(shapes)
        rows = [r for _, r in pairs]
        predicted = [i for i, (s, _) in enumerate(pairs) if s is not None and s.undecided]
        with I.IngestStream.open(ctx, 0, 0, 1, tokenizer=TOKS[tok], partition_field=field) as st:
            sets, fb = st.append_keyed(rows, finish_fallback=False)
            assert [i for i, s in enumerate(sets) if s == UND] == predicted
            keys = st.keys()
            for i, (s, _) in enumerate(pairs):
                if s is not None and not s.undecided:
                    assert keys[int(sets[i])] == s.text, s.name
            # nothing of a handed-back row is in: the ingest equals one fed the other rows only
            raw, raw_keys = PR.assign_sets([rows], field)
            assert keys == raw_keys
            assert set(predicted) <= set(int(r) for r in fb)
            counts, status = st.finish()
            desc, n_words = I.plan_desc(counts, FPR)
            # (the walkers run alike on both sides: what they hand back is finished on neither)
            ref = plain_route(ctx, [rows], raw, TOKS[tok], n_sets=len(keys), finish_fallback=False)
            same((counts, status, st.build(desc, n_words)), ref[:3], (tok, field, "nothing inserted"))
        got = keyed_route(ctx, [rows], field, TOKS[tok])
        full, full_keys = PR.assign_sets([rows], field, host_finish=True)
        assert got[3] == full_keys
        same(got, plain_route(ctx, [rows], full, TOKS[tok]), (tok, field))


@pytest.mark.parametrize("tok", TOK_IDS)
def test_three_appends_known_keys_and_host_registered_keys(ctx, tok):
    """known keys keep their sets; texts registered from the host first resolve on the device; numbering follows the first decided
    appearance: batch 2 meets "n1" at row 5 and "n0" at row 2 only after an undecided row that holds "n2" at row 0"""
    known = [b"host-a", b"", b"host-b"]
    b1 = tenant_rows(0, 70, lambda i: '"host-b"' if i % 3 else '"dev-%d"' % (i % 2))
    b2 = tenant_rows(70, 70, lambda i: '"n1"' if i >= 75 else '"host-a"')
    b2[0] = b'{"tenant":"n\\u0032","x":1}'
    b2[2] = b'{"tenant":"n0"}'
    b3 = tenant_rows(140, 70, lambda i: ['"n0"', '"n1"', '"n2"', '"dev-0"', 'null'][i % 5])
    got = keyed_route(ctx, [b1, b2, b3], "tenant", TOKS[tok], known=known)
    sets, keys = PR.assign_sets([b1, b2, b3], "tenant", known=known, host_finish=True)
    assert keys[:3] == known and keys[3:] == [b"dev-0", b"dev-1", b"n0", b"n1", b"n2"] and got[3] == keys
    assert sets[2][2] == keys.index(b"n2") and sets[2][4] == 1                               # null: the empty text, registered as set 1
    same(got, plain_route(ctx, [b1, b2, b3], sets, TOKS[tok]), tok)


def chunked_rows():
    pad = "x" * 220
    rows = tenant_rows(0, 600, lambda i: '"c%d"' % (0 if i < 200 else 1 if i < 500 else 2))
    rows = [r[:-1] + b',"pad":"' + pad.encode() + b'"}' for r in rows]
    off = np.cumsum([0] + [len(r) for r in rows])
    # 64 KiB, then 128 KiB, then the rest: a new text is first met in each of the three upload chunks
    assert off[200] > (64 << 10) and off[200] < (192 << 10) and off[500] > (192 << 10) + 512 and off[199] < (64 << 10) * 2
    return rows


@pytest.mark.parametrize("tok", TOK_IDS)
def test_upload_chunks(ctx, tok):
    rows = chunked_rows()
    ctx.set_ingest_chunk(1)                                        # the smallest: 64 KiB
    try:
        got = keyed_route(ctx, [rows], "tenant", TOKS[tok])
    finally:
        ctx.set_ingest_chunk(0)
    sets, keys = PR.assign_sets([rows], "tenant", host_finish=True)
    assert got[3] == keys == [b"c0", b"c1", b"c2"]
    same(got, plain_route(ctx, [rows], sets, TOKS[tok]), tok)


def many_key_rows():
    """more distinct new texts in one batch than the pending table holds, each twice, the second occurrences in another order; texts
    of equal length and of every length up to the cap among them"""
    n = _lib.PARTITION_PENDING_SLOTS + 44
    texts = ["k%04d" % i for i in range(n - 8)] + ["L" * m for m in (0, 1, 7, 8, 9, 127, 128, 129)]
    order = list(range(n)) + [(i * 37 + 5) % n for i in range(n)]
    base = synth.rows_json(0, 16)
    return [b'{"tenant":"' + texts[k].encode() + b'",' + base[j % 16][1:] for j, k in enumerate(order)], n


@pytest.mark.parametrize("tok", TOK_IDS)
@pytest.mark.parametrize("lab", [0, 1], ids=["hash", "hash masked to 2 bits"])
def test_more_new_keys_than_pending_slots(ctx, tok, lab):
    """every row is assigned or handed back and per-key equality holds, whatever the hash: with the lab key every lookup is decided by
    the byte compare and the texts are collected four per round"""
    rows, n = many_key_rows()
    assert n > _lib.PARTITION_PENDING_SLOTS
    ctx.set_lab(_lib.LAB_PARTITION_HASH_MASK, lab)
    try:
        got = keyed_route(ctx, [rows[:300], rows[300:]], "tenant", TOKS[tok])
    finally:
        ctx.set_lab(_lib.LAB_PARTITION_HASH_MASK, 0)
    sets, keys = PR.assign_sets([rows[:300], rows[300:]], "tenant", host_finish=True)
    assert got[3] == keys and len(keys) == n                       # ("L" * 129 is handed back and registered from the host)
    same(got, plain_route(ctx, [rows[:300], rows[300:]], sets, TOKS[tok]), (tok, lab))


@pytest.mark.parametrize("tok", TOK_IDS)
def test_the_lab_hash_mask_changes_nothing(ctx, tok):
    """the multi-key batches of the first test, the hash masked and unmasked between appends of ONE stream"""
    vals = ['"a"', '"b"', '5', '"5"', 'true', '"late"', 'null', '1.0']
    rows = tenant_rows(0, 450, lambda i: vals[(i * 7 + i // 64) % (3 + i // 90)])
    batches = [rows[:65], rows[65:322], rows[322:]]
    want, want_keys = PR.assign_sets(batches, "tenant")
    with I.IngestStream.open(ctx, 0, 0, 1, tokenizer=TOKS[tok], partition_field="tenant") as st:
        try:
            for b, rows_b in enumerate(batches):
                ctx.set_lab(_lib.LAB_PARTITION_HASH_MASK, 1 - b % 2)
                sets, fb = st.append_keyed(rows_b, finish_fallback=False)
                assert [int(s) for s in sets] == want[b] and len(fb) == 0
        finally:
            ctx.set_lab(_lib.LAB_PARTITION_HASH_MASK, 0)
        assert st.keys() == want_keys
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        same((counts, status, st.build(desc, n_words)), plain_route(ctx, batches, want, TOKS[tok])[:3], tok)


@pytest.mark.parametrize("tok", TOK_IDS)
def test_minmax_fields(ctx, tok):
    """two fields given at open: the indexes equal the route with explicit sets, the rows handed back for MinMax reasons (an exponent
    on a field, an escaped key) and the rows the partitioner handed back included"""
    fields = ["timestamp", "v"]
    rows = tenant_rows(0, 200, lambda i: '"t%d"' % (i % 4))
    for i in range(0, 200, 9):
        rows[i] = rows[i][:-1] + b',"v":%d.5}' % (i - 100)
    rows[10] = rows[10][:-1] + b',"v":1e3}'                        # MinMax hand-back, decided by the partitioner
    rows[20] = b'{"tenant":"t1","\\u0076":7,"v":-5000}'            # an escaped key BEHIND the member: partitioned, handed back by MinMax
    rows[30] = b'{"\\u0076":9000,"tenant":"t2","v":1}'             # ... in front of it: handed back by the partitioner
    rows[40] = b'{"tenant":"t\\u0033","v":-9000}'                  # an escaped value: handed back by the partitioner
    batches = [rows[:90], rows[90:]]
    with I.IngestStream.open(ctx, 0, 0, 1, tokenizer=TOKS[tok], minmax_fields=fields, partition_field="tenant") as st:
        all_sets = []
        for rows_b in batches:
            sets, fb = st.append_keyed(rows_b)
            all_sets.append([int(s) for s in sets])
            if rows_b is batches[0]:
                assert {10, 20, 30, 40} <= set(int(r) for r in fb)
        want, keys = PR.assign_sets(batches, "tenant", host_finish=True)
        assert all_sets == want and st.keys() == keys
        mm = st.minmax()
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        got = (counts, status, st.build(desc, n_words))
    ref = plain_route(ctx, batches, want, TOKS[tok], minmax_fields=fields)
    same(got, ref[:3], tok)
    for a, b in zip(mm, ref[3]):
        assert np.array_equal(a, b)
    assert mm[2].all() and int(mm[0][:, 1].min()) == -9000


@pytest.mark.parametrize("tok", TOK_IDS)
def test_a_list_that_did_not_fit_appended_again(ctx, tok):
    rows = tenant_rows(0, 120, lambda i: '"f%d"' % (i % 3))
    rows[5] = b'{"tenant":"f\\u0031"}'
    rows[50] = b'{"tenant":"esc\\\\aped"}'
    rows[77] = b'{"\\u0074enant":"f2"}'
    with I.IngestStream.open(ctx, 0, 0, 1, tokenizer=TOKS[tok], partition_field="tenant") as st:
        with pytest.raises(BloomGpuError):
            ctx.ingest_append_rows_keyed(st.id, rows, fallback_cap=1)
        assert st.keys() == [b"f0", b"f1", b"f2"] and st.stats().n_rows == 0          # the sets stay; the call that delivers the list counts the batch
        sets, n_new, fb = ctx.ingest_append_rows_keyed(st.id, rows)
        st.n_sets = 3
        assert n_new == 0 and list(fb) == [5, 50, 77] and st.stats().n_rows == 120
        want, _ = PR.assign_sets([rows], "tenant")
        assert [None if s == UND else int(s) for s in sets] == want[0]
        finish_on_host(ctx, st, rows, sets, fb, "tenant")
        full, keys = PR.assign_sets([rows], "tenant", host_finish=True)
        assert [int(s) for s in sets] == full[0] and st.keys() == keys == [b"f0", b"f1", b"f2", b"esc\\aped"]
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        same((counts, status, st.build(desc, n_words)), plain_route(ctx, [rows], full, TOKS[tok])[:3], tok)


def test_refusals_and_the_plain_calls_on_a_keyed_ingest(ctx):
    L, h = ctx.L, ctx.h
    import ctypes as C
    out = C.c_uint64()
    name = np.frombuffer(b"n" * 65, dtype=np.uint8)
    for args in ((1, 0, 0, None, C.byref(out), name.ctypes.data, 0, None, None, 0),            # an empty name
                 (1, 0, 0, None, C.byref(out), name.ctypes.data, 65, None, None, 0),           # 65 bytes
                 (1, 1, 0, None, C.byref(out), name.ctypes.data, 6, None, None, 0),            # parent 1 of 1
                 (0, 0, 0, None, C.byref(out), name.ctypes.data, 6, None, None, 0)):           # parent 0 of 0
        assert L.bsg_ingest_open_keyed(h, *args) == _lib.BSG_E_INVALID and not out.value
        assert any(w in L.bsg_last_error(h).decode() for w in ("name", "parent"))         # the cause is named
    rows = tenant_rows(0, 10, lambda i: '"a"' if i < 5 else '"b"')
    with I.IngestStream.open(ctx, 0, None, 0, partition_field="tenant") as st:      # no parents at all
        with pytest.raises(BloomGpuError):
            st.add_sets([0xFFFFFFFF])                              # a set without a text
        sets, fb = st.append_keyed(rows)
        assert list(sets) == [0] * 5 + [1] * 5 and len(fb) == 0
        assert len(st.append(rows[:3], [1, 1, 0], finish_fallback=False)) == 0      # explicit sets keep working
        sets, fb = st.append_keyed([])
        assert len(sets) == 0 and len(fb) == 0
        assert ctx.last_partition_ms() >= 0.0
        assert st.keys(1) == [b"b"] and st.keys(2) == []
        with pytest.raises(BloomGpuError):
            st.keys(3)
    with I.IngestStream.open(ctx, 1, [0], 1) as plain:
        with pytest.raises(BloomGpuError):
            ctx.ingest_append_rows_keyed(plain.id, rows)
        with pytest.raises(BloomGpuError):
            ctx.ingest_keys(plain.id)
