"""tests/survivor_row_shapes.py is what tests/test_survivor_row_edges_gpu.py judges the survivor-row kernels with; this file judges it.
The crafted arenas have exactly the designed survivors on the oracle (zero false positives: a condition on the inputs), the GPU case list
reaches both sides of every tag edge at every row width, the reference encoder and decoder of the two layouts are inverse to each other
and agree with bsg_survivor_row_list (host arithmetic), and check_call rejects seven deliberately wrong encodings of a correct call.
No GPU."""
import numpy as np
import pytest

from bloomsearch_amd.gpu import survivor_row_list
from oracle import oracle as O
from tests import helpers as H
from tests import survivor_row_shapes as S

POISON = 0xA5
POISON_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)


def test_designed_survivors_equal_the_oracle_at_every_gpu_size():
    """Zero rows may differ.  Should a string ever collide, change S.FILLER, not this assertion."""
    for B in S.all_block_counts():
        p = S.plan(B)
        assert p.n_blocks == B and set(int(k) for k in p.desc["k"][1::3]) <= {20, 21}
        got = O.survivors_tree(H.oracle_words(p), p.desc.view(O.DESC_DTYPE), S.BASE_EXPRS)
        assert np.array_equal(S.bits_to_matrix(got, B), S.design_matrix(B)), B


def test_patterns_are_the_counts_and_places_of_the_design():
    assert sorted(S.COUNTS) == sorted(("0", "1", "2", "2G-1", "2G", "2G+1", "2G+2", "B/2", "B-1", "B")) and len(S.PATTERNS) == 30
    for B in (1, 2, 3, 63, 64, 65, 321, 1024, 1153):
        M, G = S.design_matrix(B), S.words_of(B)
        for j, (sym, place) in enumerate(S.PATTERNS):
            c = S.count_of(sym, B)
            assert 0 <= c <= B and M[j].sum() == c, (B, sym, place)
            if c and place == "last":
                assert M[j, B - 1] and M[j, B - c]
            if c and place == "first":
                assert M[j, 0] and M[j, c - 1]
            if place == "spread" and c >= 2 * G and B % 64 == 0:
                assert len(set(np.flatnonzero(M[j]) // 64)) == G, (B, sym)          # every word of the row takes part
        assert M[-1].all()


def test_stretch_cycles_with_a_rotation():
    assert S.stretch(S.N_BASE).tolist() == list(range(S.N_BASE))
    for NQ in (257, 513):
        idx = S.stretch(NQ)
        assert set(idx.tolist()) == set(range(S.N_BASE))
        assert not np.array_equal(idx[: S.N_BASE], idx[S.N_BASE: 2 * S.N_BASE])
    # rows on either side of a 256-query boundary carry different tags, and at the first boundary both carry a payload
    for B in (64, 321, 1024, 1153):
        M = S.design_matrix(B)[S.stretch(513)]
        tags = [S.tag_of(int(c), B) for c in M.sum(axis=1)]
        assert {tags[255], tags[256]} == {S.TAG_DENSE, S.TAG_LIST} and tags[511] != tags[512], (B, tags[255], tags[256], tags[511], tags[512])


@pytest.mark.parametrize("G", list(range(1, 17)) + [17])
def test_gpu_cases_reach_both_sides_of_every_tag_edge(G):
    hits = [(B, NQ) for nbs, NQ in S.gpu_cases() for B in nbs if S.words_of(B) == G and B > 2 * G + 1]
    assert hits, G
    for B, NQ in hits:
        counts = S.design_matrix(B)[S.stretch(NQ)].sum(axis=1).tolist()
        if NQ >= S.N_BASE:
            assert {0, 1, 2 * G, 2 * G + 1, B - 1, B} <= set(counts), (B, NQ)
    B, NQ = max(hits, key=lambda h: h[1])
    assert NQ >= S.N_BASE
    assert [S.tag_of(c, B) for c in (0, 1, 2 * G, 2 * G + 1, B - 1, B)] == [S.TAG_NONE, S.TAG_LIST, S.TAG_LIST, S.TAG_DENSE, S.TAG_DENSE, S.TAG_ALL]


def test_gpu_case_list_is_the_one_the_edges_were_chosen_for():
    assert sorted(set(S.words_of(B) for B in S.WIDTH_BS)) == list(range(1, 17)) and len(S.WIDTH_BS) == 48
    assert [S.words_of(B) for B in S.UNSTAGED_BS] == [17, 17, 19] and [S.words_of(B) for B in S.QEDGE_BS] == [1, 6, 16]
    for B in S.UNSTAGED_BS:      # every tag occurs on the path without the tile
        tags = {S.tag_of(int(c), B) for c in S.design_matrix(B)[S.stretch(S.UNSTAGED_NQ)].sum(axis=1)}
        assert tags == {0, 1, 2, 3}, B
    assert S.tag_of(1, 1) == S.TAG_ALL and S.tag_of(2, 2) == S.TAG_ALL and S.tag_of(1, 2) == S.TAG_LIST     # ALL wins over LIST
    assert [len(S.run_blocks(n)) for n in S.RUN_ARENAS] == [63, 64, 65, 129] and S.RUN_NQ >= S.N_BASE
    L = S.Layout(S.SHARD_BS + (S.SHARD_REFUSED_B,), S.SHARD_NQ, S.SHARD_ND)
    assert [u.nl for u in L.units] == [1024, 961, 1025, 1024, 961, 1024, 1024, 961, 1024]


def _designed(nbs, NQ):
    return [S.design_matrix(B)[S.stretch(NQ)] for B in nbs]


@pytest.mark.parametrize("packed", [False, True])
def test_reference_encoder_and_decoder_are_inverse(packed):
    single = [B for B in S.all_block_counts() if packed is False or B <= 1024]
    calls = [(single, S.N_BASE, 1), (list(S.QEDGE_BS), 513, 1), (list(S.SHARD_BS) + ([] if packed else [S.SHARD_REFUSED_B]), S.SHARD_NQ, S.SHARD_ND)]
    for nbs, NQ, nd in calls:
        want = _designed(nbs, NQ)
        enc = S.encode_call(nbs, NQ, want, packed, POISON, nd)
        ids, tags = S.decode_call(enc.rows, enc.hdr, nbs, NQ, packed, nd)
        for i in range(len(nbs)):
            for q in range(NQ):
                assert np.array_equal(ids[i][q], np.flatnonzero(want[i][q])), (nbs[i], q, nd)
        if nd == 1 and NQ == S.N_BASE:
            assert all(set(tags[(0, i)].tolist()) == {0, 1, 2, 3} for i, B in enumerate(nbs) if B >= 4)
        S.check_call(enc.rows, enc.hdr, POISON, nbs, NQ, want, packed, nd, enc.layout.row_words, enc.layout.hdr_count)


def test_bsg_survivor_row_list_reads_every_reference_row():
    """The library's host-side reader (no device) returns the designed ids for every dense-layout row of the reference encoder."""
    nbs = [B for B in S.all_block_counts() if B <= 1153]
    want = _designed(nbs, S.N_BASE)
    enc = S.encode_call(nbs, S.N_BASE, want, False, POISON)
    for u in enc.layout.units:
        for q in range(S.N_BASE):
            got = survivor_row_list(int(enc.hdr[u.hdr_at + q]), enc.rows[u.row_off + q * u.G: u.row_off + (q + 1) * u.G], u.nl)
            assert np.array_equal(got, np.flatnonzero(want[u.i][q])), (u.nl, q)


# ---- check_call must notice: seven wrong encodings of an otherwise correct call ----
NBS, NQ = [64, 321], 257          # G = 1 and 6; two runs of queries
TAIL = 4


def _correct(packed):
    want = _designed(NBS, NQ)
    L = S.Layout(NBS, NQ)
    enc = S.encode_call(NBS, NQ, want, packed, POISON, 1, L.row_words + TAIL, L.hdr_count + TAIL)
    return want, enc, enc.rows.copy(), enc.hdr.copy()


def _check(rows, hdr, want, packed):
    L = S.Layout(NBS, NQ)
    S.check_call(rows, hdr, POISON, NBS, NQ, want, packed, 1, L.row_words, L.hdr_count)


def _row(want, enc, i, count):
    """(unit, query) of the first row of arena i with `count` survivors."""
    q = int(np.flatnonzero(want[i].sum(axis=1) == count)[0])
    return enc.layout.units[i], q


def _list_only_below_2g(want, enc, rows, hdr):
    u, q = _row(want, enc, 1, 12)                            # count == 2 G: a LIST row; `count < 2 G` would write it DENSE
    hdr[u.hdr_at + q] = (S.TAG_DENSE << 30) | 12
    rows[u.row_off + q * u.G: u.row_off + (q + 1) * u.G] = S._row_words(want[1][q], u.G)


def _full_row_tagged_dense(want, enc, rows, hdr):
    u, q = _row(want, enc, 0, 64)
    hdr[u.hdr_at + q] = (S.TAG_DENSE << 30) | 64
    rows[u.row_off + q] = ~np.uint64(0)


def _none_slot_zeroed(want, enc, rows, hdr):
    u, q = _row(want, enc, 1, 0)
    rows[u.row_off + q * u.G: u.row_off + (q + 1) * u.G] = 0


def _run_starts_one_word_late(want, enc, rows, hdr):
    start, total = enc.runs[(0, 1, 0)]
    assert 0 < total < 256 * 6
    rows[start + 1: start + 1 + total] = rows[start: start + total].copy()
    rows[start] = POISON_WORD


def _second_run_continues_the_first(want, enc, rows, hdr):
    (s0, t0), (s1, t1) = enc.runs[(0, 1, 0)], enc.runs[(0, 1, 1)]
    assert t1 > 0 and s0 + t0 < s1
    rows[s0 + t0: s0 + t0 + t1] = rows[s1: s1 + t1].copy()
    rows[s1: s1 + t1] = POISON_WORD


def _ids_descending(want, enc, rows, hdr):
    u, q = _row(want, enc, 1, 11)
    ids = rows[u.row_off + q * u.G: u.row_off + (q + 1) * u.G].view(np.uint32)
    ids[:11] = ids[:11][::-1].copy()


def _word_past_the_used_part(want, enc, rows, hdr):
    rows[enc.layout.row_words] = 0


WRONG = [(False, _list_only_below_2g), (False, _full_row_tagged_dense), (False, _none_slot_zeroed), (True, _none_slot_zeroed),
         (True, _run_starts_one_word_late), (True, _second_run_continues_the_first), (False, _ids_descending),
         (False, _word_past_the_used_part), (True, _word_past_the_used_part)]


@pytest.mark.parametrize("packed,mutate", WRONG, ids=["%s-%s" % (m.__name__.strip("_"), "packed" if p else "dense") for p, m in WRONG])
def test_check_call_rejects_a_wrong_encoding(packed, mutate):
    want, enc, rows, hdr = _correct(packed)
    _check(rows, hdr, want, packed)                          # the call as it should be passes ...
    mutate(want, enc, rows, hdr)
    assert not (np.array_equal(rows, enc.rows) and np.array_equal(hdr, enc.hdr))
    with pytest.raises(AssertionError):                      # ... and the one deviation does not
        _check(rows, hdr, want, packed)


def test_check_call_rejects_more_that_the_header_forbids():
    """Beyond the seven: a header written behind the last one, a count in a packed header that is not a LIST, a size report that is off."""
    for packed in (False, True):
        want, enc, rows, hdr = _correct(packed)
        h8 = hdr.view(np.uint8)
        h8[enc.layout.hdr_count * (1 if packed else 4)] = 0
        with pytest.raises(AssertionError):
            _check(rows, hdr, want, packed)
        with pytest.raises(AssertionError):
            S.check_call(enc.rows, enc.hdr, POISON, NBS, NQ, want, packed, 1, enc.layout.row_words + 1, enc.layout.hdr_count)
    want, enc, rows, hdr = _correct(True)
    u, q = _row(want, enc, 1, 321)
    hdr.view(np.uint8)[u.hdr_at + q] |= 1                    # an ALL row's packed header carries no count
    with pytest.raises(AssertionError):
        _check(rows, hdr, want, True)
    # the dense layout's LIST row may leave anything behind its ids INSIDE its slot: not an error
    want, enc, rows, hdr = _correct(False)
    u, q = _row(want, enc, 1, 1)
    rows[u.row_off + q * u.G + 1: u.row_off + (q + 1) * u.G] = 0
    rows[u.row_off + q * u.G: u.row_off + q * u.G + 1].view(np.uint32)[1] = 7
    _check(rows, hdr, want, False)
