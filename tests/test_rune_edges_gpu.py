"""The rune path of the device walkers, exactly: every case pair, every UTF-8 length-class edge, the lower table's own edge, every range of
code points the tables do not know, every byte phase of a multi-byte rune, every case of the n-gram ring, the text consumers, runes in keys
and every kind of text that must go to the host — the shape families of tests/rune_shapes.py through device_ingest, match_rows_lookup,
match_rows_lookup_rows, match_rows, match_rows_substr and match_rows_regex.

Every expectation is the shape module's closed form (tests/test_rune_shapes.py proves it equal to the restatements and the host mirror):
counts, bitsets (the oracle's build of the expected sets, word for word), verdict matrices bit for bit, and the FALLBACK LIST EXACTLY — the
rows holding an unknown code point below U+20000 under a lowering spec, none under a raw one, none in families B and C."""
import numpy as np
import pytest

from bloomsearch_amd import host as Hst, ingest as I, query as Q
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from tests import rune_shapes as S
from tests import substring_restatement as SR
from tests import tokenizer_restatement as TR
from tests.test_tokenizer_ingest_gpu import FPR, check

pytestmark = pytest.mark.gpu


def names_of(rows, indices):
    return [rows[i].name for i in sorted(indices)[:6]]


def ingest_check(ctx, sets_of_rows, spec, tok, expect_back=None):
    """one device_ingest call, one set per list of Rows: the fallback list exactly, then counts and bitsets of every set"""
    flat = [r for rows in sets_of_rows for r in rows]
    res = I.device_ingest(ctx, [[r.row for r in rows] for rows in sets_of_rows], FPR, tokenizer=tok)
    want_back = [i for i, r in enumerate(flat) if S.hands_back(r.cps, spec)] if expect_back is None else expect_back
    got_back = [int(x) for x in res.fallback_rows]
    assert got_back == want_back, ("handed back and not expected", names_of(flat, set(got_back) - set(want_back)),
                                   "expected and not handed back", names_of(flat, set(want_back) - set(got_back)))
    assert not np.asarray(res.status).any()
    for s, rows in enumerate(sets_of_rows):
        words = {t for r in rows for t in S.word_tokens(r.cps, spec)}
        pairs = {r.key + "::" + t for r in rows for t in S.word_tokens(r.cps, spec)}
        check(res, s, ({r.key for r in rows}, words, pairs), rows[0].name + " .. " + rows[-1].name)


def lookup_check(ctx, rows, spec, tok, conds=None):
    """match_rows_lookup and match_rows_lookup_rows over `rows` with one FieldToken query per entry of conds ((key, token); default: the
    first token of every row, the row's own text where it has none): every pair bit for bit, the fallback list exactly"""
    toks = [S.word_tokens(r.cps, spec) for r in rows]
    if conds is None:
        conds = [(r.key, t[0] if t else "".join(chr(c) for c in r.cps)) for r, t in zip(rows, toks)]
    want_back = [i for i, r in enumerate(rows) if S.hands_back(r.cps, spec)]
    holders = {}
    for i, (r, t) in enumerate(zip(rows, toks)):
        if i not in set(want_back):
            for x in set(t):
                holders.setdefault((r.key, x), []).append(i)
    want = np.zeros((len(conds), len(rows)), dtype=bool)
    for q, c in enumerate(conds):
        want[q, holders.get(c, [])] = True
    batch = Q.CompiledLookupBatch([Q.FieldToken(k, t) for k, t in conds])
    assert len(batch.kinds) <= 1024 and len(rows) <= 1024 and batch.n_queries == len(conds)
    raw = [r.row for r in rows]
    words, pwo, fb = ctx.match_rows_lookup(raw, batch, tokenizer=tok)
    hdr, poff, payload, fb_rows = ctx.match_rows_lookup_rows(raw, batch, tokenizer=tok)
    for got_back in ([int(x) for x in fb], [int(x) for x in fb_rows]):
        assert got_back == want_back, ("handed back and not expected", names_of(rows, set(got_back) - set(want_back)),
                                       "expected and not handed back", names_of(rows, set(want_back) - set(got_back)))
    got = np.array([wide_pair_bits(words, pwo, q, len(rows)) for q in range(len(conds))])
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(conds[q], rows[r].name, bool(want[q, r])) for q, r in bad[:6]]
    for q in range(len(conds)):
        listed = pair_rows_list(int(hdr[q]), payload[int(poff[q]): int(poff[q + 1])], len(rows))
        assert np.array_equal(listed, np.flatnonzero(want[q])), (conds[q], names_of(rows, set(map(int, listed)) ^ set(np.flatnonzero(want[q]))))
    return want


# ---------------- family A: the code-point sweep ----------------
A_CHUNKS = S.sweep_chunks()


@pytest.mark.parametrize("chunk", range(len(A_CHUNKS)))
@pytest.mark.parametrize("name", S.A_SPECS)
def test_sweep_ingest(ctx, name, chunk):
    """one set per 64 code points (256 rows): a failure names its code points"""
    spec, tok = S.SPECS[name]
    cps = A_CHUNKS[chunk]
    ingest_check(ctx, [S.sweep_rows(cps[i:i + 64]) for i in range(0, len(cps), 64)], spec, tok)


@pytest.mark.parametrize("chunk", range(len(A_CHUNKS)))
@pytest.mark.parametrize("name", S.A_SPECS)
def test_sweep_match_lookup(ctx, name, chunk):
    """256 code points (1 024 rows, one condition each) per call: the identity and the coincidences of two code points lowering to one"""
    spec, tok = S.SPECS[name]
    cps = A_CHUNKS[chunk]
    hits = 0
    for i in range(0, len(cps), 256):
        hits += int(lookup_check(ctx, S.sweep_rows(cps[i:i + 256]), spec, tok).sum())
    assert hits >= len(cps)


# ---------------- family B: byte phase ----------------
@pytest.mark.parametrize("name", S.B_SPECS)
def test_byte_phase(ctx, name):
    spec, tok = S.SPECS[name]
    rows = [r for r, _, _ in S.phase_rows()]
    ingest_check(ctx, [[r] for r in rows], spec, tok, expect_back=[])
    conds = sorted({(r.key, t) for r in rows for t in S.word_tokens(r.cps, spec)})
    for i in range(0, len(conds), 1024):
        assert lookup_check(ctx, rows, spec, tok, conds[i:i + 1024]).any(axis=1).all()


@pytest.mark.parametrize("name", S.B_SPECS)
def test_byte_phase_with_the_row_last_in_the_buffer(ctx, name):
    """each row is its call's whole buffer and its string ends on the rune: the bytes the walker has loaded beyond the row's end are never read as text"""
    spec, tok = S.SPECS[name]
    for cp in S.B_RUNES:
        for spell in ("raw", "escaped"):
            for phase in range(8):
                r = S.alone_phase_row(cp, phase, spell)
                toks = S.word_tokens(r.cps, spec)
                assert toks == ["w" + chr(cp)]
                for token, want in ((toks[0], True), ("w", False), (toks[0] + '"', False), (toks[0] + '"}', False)):
                    hits, fb = ctx.match_rows([r.row], Q.CompiledMatcher(Q.FieldToken(r.key, token)), tok)
                    assert len(fb) == 0 and [bool(x) for x in hits] == [want], (r.name, token)
                if phase in (1, 6):
                    ingest_check(ctx, [[r]], spec, tok, expect_back=[])


# ---------------- family C: the n-gram ring ----------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_ring_ingest(ctx, n):
    rows = S.ring_rows(n)
    ingest_check(ctx, [rows[i:i + 256] for i in range(0, len(rows), 256)], S.RING_SPECS[n], S.RING_SPECS[n], expect_back=[])


@pytest.mark.parametrize("quarter", range(4))
@pytest.mark.parametrize("n", [2, 3, 4])
def test_ring_match_lookup(ctx, n, quarter):
    """every window of a word is a condition that matches its own row only"""
    spec = S.RING_SPECS[n]
    rows = S.ring_rows(n)
    rows = rows[quarter * len(rows) // 4: (quarter + 1) * len(rows) // 4]
    for i in range(0, len(rows), 341):
        part = rows[i:i + 341]
        conds = [(r.key, t) for r in part for t in S.word_tokens(r.cps, spec)]
        want = lookup_check(ctx, part, spec, spec, conds)
        assert want.shape == (3 * len(part), len(part)) and (want.sum(axis=1) == 1).all() and (want.sum(axis=0) == 3).all()


@pytest.mark.parametrize("name,n", [("tri_default", 3), ("four_nosep_lower", 4)])
def test_ring_sees_the_lowered_length(ctx, name, n):
    spec, tok = S.SPECS[name]
    rows = S.lowered_rows(n)
    ingest_check(ctx, [rows[i:i + 256] for i in range(0, len(rows), 256)], spec, tok, expect_back=[])
    for i in range(0, len(rows), 256):
        part = rows[i:i + 256]
        conds = sorted({(r.key, t) for r in part for t in S.word_tokens(r.cps, spec)})
        assert lookup_check(ctx, part, spec, tok, conds).any(axis=1).all()


# ---------------- family D: the text consumers ----------------
UNKNOWN_CP = S.unknown_ranges()[0][0]


@pytest.mark.parametrize("walker", ["default", "trigram"])
def test_substring_consumer_folds_the_rune(ctx, walker):
    tok = SR.WALKERS[walker]
    cases = S.substring_rows()
    unknown = S.make_row(b"ab" + S.utf8(UNKNOWN_CP) + b"cd", (), "unknown", b"t").row
    rows = [r.row for r, _, _ in cases] + [unknown]
    for r, hit, miss in cases[::2]:                              # the raw and the escaped row of a code point share their needles
        for needle, expect in ((hit, True), (miss, False)):
            e = Q.FieldSubstring("t", needle)
            want = np.array([SR.row_verdict(x, e, tok) for x in rows[:-1]] + [False])
            assert want[rows.index(r.row)] == expect and want.sum() >= 2 * expect
            hits, fb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(None, e), tok)
            assert [int(x) for x in fb] == [len(rows) - 1], (r.name, needle)     # the unknown code point: the host's, and nowhere else
            assert np.array_equal(hits, want), (r.name, needle, np.flatnonzero(hits != want)[:6])


def test_regex_consumer_is_fed_the_original_rune(ctx):
    cps = S.REGEX_CODE_POINTS
    rows = [S.make_row(b"ab" + text + b"cd", (), "", b"t").row for cp in cps for text in (S.utf8(cp), S.escaped(cp, True))]
    for j, cp in enumerate(cps):
        for literal, want in ((cp, [i // 2 == j for i in range(len(rows))]), (S.lower(cp), [False] * len(rows))):
            e = Q.FieldRegex("t", "b" + chr(literal) + "c")
            assert [TR.row_verdict(r, S.DEFAULT, None, e) for r in rows] == want
            hits, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, e))
            assert len(fb) == 0 and [bool(x) for x in hits] == want, "U+%04X literal U+%04X" % (cp, literal)


# ---------------- family E: runes in keys ----------------
def test_keys_are_copied_and_never_lowered(ctx):
    cases = S.key_rows()
    rows = [row for row, _, _ in cases]
    for row, hit, miss in cases[::3]:
        for field in (hit, miss):
            want = [h == field for _, h, _ in cases]             # the three spellings of the key name one path
            assert [TR.row_verdict(r, S.DEFAULT, Q.Field(field)) for r in rows] == want and any(want) == (field == hit)
            hits, fb = ctx.match_rows(rows, Q.CompiledMatcher(Q.Field(field)))
            assert len(fb) == 0 and [bool(x) for x in hits] == want, field


def test_an_escaped_rune_at_the_path_cap(ctx):
    cases = S.key_cap_rows()
    rows = [row for row, _, _ in cases]
    outside = [i for i, (_, longest, _) in enumerate(cases) if longest > S.PATH_CAP]
    assert len(outside) == len(cases) // 2
    for _, _, field in cases[::2]:
        want = [f == field and i not in outside for i, (_, _, f) in enumerate(cases)]
        hits, fb = ctx.match_rows(rows, Q.CompiledMatcher(Q.Field(field)))
        assert [int(x) for x in fb] == outside and [bool(x) for x in hits] == want, field
        assert [Hst.match_row(Q.Field(field), r) for r in rows] == [f == field for _, _, f in cases]
    res = I.device_ingest(ctx, [[r] for r in rows], FPR)
    assert [int(x) for x in res.fallback_rows] == outside
    for i, (row, _, field) in enumerate(cases):
        check(res, i, ({field}, {"value"}, {field + "::value"}), field)


# ---------------- family F: what must be handed back ----------------
@pytest.mark.parametrize("name", ["default", "punct_lower"])
def test_invalid_text_is_handed_back_and_its_valid_neighbour_is_not(ctx, name):
    spec, tok = S.SPECS[name]
    faults = [f for f in S.fault_rows() if not f.documented_only]
    rows = [f.row for f in faults]
    want_back = [i for i, f in enumerate(faults) if f.handed_back]
    assert 20 < len(want_back) < len(faults) - 10
    res = I.device_ingest(ctx, [[r] for r in rows], FPR, tokenizer=tok)
    got_back = [int(x) for x in res.fallback_rows]
    assert got_back == want_back, [faults[i].name for i in set(got_back) ^ set(want_back)]
    for i, f in enumerate(faults):                               # the host has finished the handed-back rows: U+FFFD for each invalid byte
        toks = {t.decode("utf-8") for t in TR.tokens(S.fault_text(f.row), spec)}
        check(res, i, ({"v"}, toks, {"v::" + t for t in toks}), f.name)
    hits, fb = ctx.match_rows(rows, Q.CompiledMatcher(Q.Field("v")), tok)
    assert [int(x) for x in fb] == want_back and [bool(x) for x in hits] == [not f.handed_back for f in faults]


def test_an_escape_cut_short_is_handed_back_or_no_row(ctx):
    """three hex digits and the closing quote: no valid JSON.  The documented verdict is "handed back or not a row": its bit is false
    either way, and its valid neighbours in the same call are decided"""
    (cut,) = [f for f in S.fault_rows() if f.documented_only]
    rows = [b'{"v":"a\\u0041"}', cut.row, b'{"v":"a\\u004a"}']
    hits, fb = ctx.match_rows(rows, Q.CompiledMatcher(Q.Field("v")))
    assert [bool(x) for x in hits] == [True, False, True] and set(int(x) for x in fb) <= {1}
