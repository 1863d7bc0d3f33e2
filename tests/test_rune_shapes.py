"""tests/rune_shapes.py kept honest on the CPU: the pinned counts of the case pairs and of the unknown code points, the closed forms
against the restatements (tests/tokenizer_restatement.py, tests/ngram_restatement.py, tests/substring_restatement.py) and against the
host mirror (bloomsearch_amd.host), the fallback expectations from the stated rule alone, every row inside the walker's envelope, the
byte phases of family B, and the coverage of gram_push's cases by the words of family C.  No GPU."""
import json
import unicodedata
from collections import Counter

import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import ngram_restatement as NR
from tests import rune_shapes as S
from tests import substring_restatement as SR
from tests import tokenizer_restatement as TR
from tests import walker_envelope_shapes as ENV


def text_of(r: S.Row) -> str:
    return "".join(chr(c) for c in r.cps)


# ---------------- the pinned counts ----------------
def test_the_case_pairs_are_1407_with_the_stated_length_histogram():
    pairs = S.case_pairs()
    assert len(pairs) == S.N_PAIRS == 1407
    assert Counter((len(S.utf8(a)), len(S.utf8(b))) for a, b in pairs) == S.LENGTH_HISTOGRAM
    assert sum(S.LENGTH_HISTOGRAM.values()) == 1407
    changing = S.length_changing()
    assert len(changing) == 25 and 0x130 in changing         # U+0130 is one of the 25 (the 2 -> 1)
    assert {0x23A, 0x23E, 0x1E9E, 0x2126, 0x212A, 0x212B} <= set(changing)
    assert len([cp for cp in changing if len(S.utf8(cp)) == 3 and len(S.utf8(S.lower(cp))) == 2]) == 21
    assert len(S.four_byte_block_ends()) >= 14                  # seven scripts, both ends of each run of capitals


def test_the_unknown_ranges_are_634_with_44137_code_points():
    ranges = S.unknown_ranges()
    assert len(ranges) == S.N_UNKNOWN_RANGES == 634 and len(S.unknown_set()) == S.N_UNKNOWN == 44137
    assert all(a <= b for a, b in ranges) and all(b + 1 < a2 for (_, b), (a2, _) in zip(ranges, ranges[1:]))
    assert ranges[0][0] >= 0x80 and ranges[-1][1] < S.TABLE_END
    in_pair = {c for p in S.case_pairs() for c in p}
    assert not in_pair & S.unknown_set()                        # "not in a 14.0 case pair": neither side of any pair


@pytest.mark.skipif(unicodedata.unidata_version != "13.0.0", reason="the rule is stated over Unicode 13.0.0")
def test_the_committed_ranges_are_the_rule_over_unicode_13():
    assert [tuple(r) for r in S.derive_unknown_ranges()] == list(S.unknown_ranges())


def test_the_host_mirror_leaves_every_unknown_code_point_unchanged():
    cps = sorted(S.unknown_set())
    for i in range(0, len(cps), 2048):
        part = cps[i:i + 2048]
        assert Hst.tokenize(" ".join("A" + chr(c) for c in part)) == ["a" + chr(c) for c in part]


def test_the_sweep_holds_what_the_issue_lists():
    cps = set(S.sweep_code_points())
    assert all(a in cps and b in cps for a, b in S.case_pairs())
    assert set(S.UTF8_EDGES) <= cps and len(S.UTF8_EDGES) == 20
    assert len(S.SPACES) == 19 and set(S.SPACES) <= cps and {0x84, 0x86, 0x9F, 0xA1, 0x1FFF, 0x200B, 0x2FFF, 0x3001} <= cps
    for a, b in S.unknown_ranges():
        assert {c for c in (a - 1, a, b, b + 1) if not 0xD800 <= c <= 0xDFFF} <= cps      # D7FF ends a range: U+D800 is family F's
    assert not any(0xD800 <= cp <= 0xDFFF for cp in cps) and min(cps) < 0x80            # 'k' and 'i': images of U+212A and U+0130
    assert all(len(c) <= S.A_CHUNK and len(c) * 4 <= 6144 for c in S.sweep_chunks())
    assert sum(len(c) for c in S.sweep_chunks()) == len(cps)


# ---------------- closed forms, restatements and the host mirror ----------------
def all_rows():
    """(family, Row) of every row the GPU tests decide with word_tokens / hands_back"""
    for r in S.sweep_rows(S.sweep_code_points()):
        yield "A", r
    for r, _, _ in S.phase_rows():
        yield "B", r
    for cp in S.B_RUNES:
        for phase in range(8):
            for spell in ("raw", "escaped"):
                yield "B", S.alone_phase_row(cp, phase, spell)
    for n in (2, 3, 4):
        for r in S.ring_rows(n):
            yield "C%d" % n, r
    for n in (3, 4):
        for r in S.lowered_rows(n):
            yield "CL%d" % n, r


SPECS_OF = {"A": S.A_SPECS, "B": S.B_SPECS, "C2": [2], "C3": [3], "C4": [4], "CL3": ["tri_default"], "CL4": ["four_nosep_lower"]}


def spec_named(name):
    return S.RING_SPECS[name] if isinstance(name, int) else S.SPECS[name][0]


def test_every_row_is_one_leaf_holding_its_code_points():
    """valid JSON, valid UTF-8, the one member's decoded text is the row's code points: raw and escaped spellings alike"""
    n = 0
    for _, r in all_rows():
        assert TR.leaves(r.row) == [(r.key, True, text_of(r))], r.name
        r.row.decode("utf-8", "strict")
        n += 1
    assert n > 30000


def test_the_closed_forms_are_the_restatements_and_the_host_mirrors():
    seen = {}
    for family, r in all_rows():
        for name in SPECS_OF[family]:
            key = (name, r.cps)
            if key in seen:                                     # the raw and the escaped spelling decode to one text
                continue
            spec = spec_named(name)
            want = [t.encode("utf-8") for t in S.word_tokens(r.cps, spec)]
            seen[key] = True
            assert NR.tokens(text_of(r), spec) == want, (r.name, name)
            assert Hst.tokenize(text_of(r), spec, as_bytes=True) == want, (r.name, name)
    assert len(seen) > 80000


def test_the_host_mirror_walks_the_escaped_rows_as_the_closed_form_says():
    """bsh_entry_sets_index_row_with and bsh_match_row_with on whole rows: sets of 64 code points, as the device test ingests them"""
    cps = S.sweep_code_points()
    for name in S.A_SPECS:
        spec, tok = S.SPECS[name]
        for i in range(0, len(cps), 64):
            rows = S.sweep_rows(cps[i:i + 64])
            es = Hst.EntrySets()
            for r in rows:
                es.index_row(r.row, tok)
            words = {t for r in rows for t in S.word_tokens(r.cps, spec)}
            assert es.as_python_sets() == ({"v"}, words, {"v::" + t for t in words}), (name, hex(cps[i]))
        for r in S.sweep_rows(cps[::16]):
            toks = S.word_tokens(r.cps, spec)
            assert Hst.match_row(Q.FieldToken("v", toks[0] if toks else text_of(r)), r.row, tok) == bool(toks), (r.name, name)


def test_separators_reached_by_lowering_split_the_word():
    k, i = (ord("x"), 0x212A, ord("y")), (ord("x"), 0x130, ord("y"))
    assert S.word_tokens(k, S.K_SEP) == ["x", "y"] and S.word_tokens(k, S.I_SEP) == ["xky"] and S.word_tokens((0x212A,), S.K_SEP) == []
    assert S.word_tokens(i, S.I_SEP) == ["x", "y"] and S.word_tokens(i, S.K_SEP) == ["xiy"]
    assert S.word_tokens(k, TR.SPECS["punct_raw"]) == ["xKy"]
    assert S.word_tokens((ord("x"), 0x3000, ord("y")), S.DEFAULT) == ["x", "y"]
    assert S.word_tokens((ord("x"), 0x3000, ord("y")), NR.SPECS["four_nosep_lower"]) == ["x　y"]


# ---------------- the fallback expectations ----------------
def test_the_fallback_lists_follow_from_the_rule_alone():
    """a row is expected back exactly when the spec lowers and a code point of its text is below U+20000 and in the committed list;
    both outcomes occur under every lowering spec, none under a raw one, and nothing at or above the table's end counts"""
    rows = S.sweep_rows(S.sweep_code_points())
    for name in S.A_SPECS:
        spec = S.SPECS[name][0]
        back = [r for r in rows if S.hands_back(r.cps, spec)]
        if not spec.lower:
            assert name == "punct_raw" and not back
            continue
        assert len(back) == 4 * len([cp for cp in S.sweep_code_points() if S.is_unknown(cp)]) > 4 * 634
        assert all(any(S.is_unknown(cp) and cp < S.TABLE_END for cp in r.cps) for r in back)
    assert not any(S.is_unknown(cp) for cp in (0x1FFFF, 0x20000, 0x2FFFF, 0xFFFF, 0xFFFD, 0xE000))
    for family, r in all_rows():
        if family != "A":
            assert not any(S.is_unknown(cp) for cp in r.cps), r.name         # families B and C expect empty lists


def test_no_row_leaves_the_envelope_for_another_reason():
    """depth 1, paths far below the cap, no DEL, no control byte, no escape but \\uXXXX, no raw byte the walker refuses"""
    for _, r in all_rows():
        assert ENV.measure(r.row) == (len(r.key), 1) and 1 <= len(r.key) <= 8, r.name
        body = r.row[len(r.key) + 5:-2]
        assert r.row == b'{"' + r.key.encode() + b'":"' + body + b'"}'
        assert not any(b < 0x20 or b == 0x7F or b == 0x22 for b in body), r.name
        assert b"\\" not in body.replace(b"\\u", b""), r.name
    for row, longest, _ in S.key_cap_rows():
        assert ENV.measure(row) == (longest, 1)
        assert ENV.in_envelope(row) == (longest <= S.PATH_CAP)
    assert sorted({longest for _, longest, _ in S.key_cap_rows()}) == [S.PATH_CAP, S.PATH_CAP + 1]


# ---------------- family B ----------------
def test_the_phase_rows_put_the_rune_at_every_phase():
    for start in (0, 3):
        rows = S.phase_rows(start)
        blob = b"\0" * start + b"".join(r.row for r, _, _ in rows)
        seen = set()
        for r, off, phase in rows:
            assert off % 8 == phase and (blob[off] >= 0xC2 or blob[off:off + 2] == b"\\u"), r.name
            assert blob[off - 1:off] in (b'"', b"w", b"j") and 1 <= len(r.key) <= 8
            seen.add((r.cps[-1 if " last " in r.name else (0 if " first " in r.name else len(S.RUN_A))], "raw" if blob[off] >= 0xC2 else "esc",
                      r.name.split()[2], phase))
        assert len(seen) == 3 * 2 * 3 * 8 == len(rows)
    assert len(S.escaped(0x1F600, True)) == 12 and len(S.RUN_A) >= 8 and len(S.RUN_B) >= 8
    for cp in S.B_RUNES:
        for phase in range(8):
            r = S.alone_phase_row(cp, phase)
            off = r.row.index(S.utf8(cp))
            assert off % 8 == phase and r.row.endswith(S.utf8(cp) + b'"}')
    ends = {(len(r.row) - 2 - 1) // 8 == (len(r.row) - 1) // 8 for cp in S.B_RUNES for phase in range(8) for r in [S.alone_phase_row(cp, phase)]}
    assert ends == {True, False}                                # the rune's last byte in the buffer's final 8-byte word, and before it


# ---------------- family C ----------------
def test_the_ring_words_are_all_of_them_with_windows_of_their_own():
    assert [len(S.ring_words(n)) for n in (2, 3, 4)] == [4 ** 4, 4 ** 5, 4 ** 6] and sum(len(S.ring_words(n)) for n in (2, 3, 4)) == 5376
    for n in (2, 3, 4):
        spec, owner = S.RING_SPECS[n], {}
        assert spec.ngram == n
        for w, (lens, cps) in enumerate(S.ring_words(n)):
            assert len(cps) == n + 2 and tuple(len(S.utf8(c)) for c in cps) == lens
            toks = S.word_tokens(cps, spec)
            assert len(toks) == 3 == len(set(toks))
            assert toks == ["".join(chr(c) for c in cps[i:i + n]) for i in range(3)]       # no rune lowered, none a separator
            for t in toks:
                assert owner.setdefault(t, w) == w, (n, lens, t)
        assert len({lens for lens, _ in S.ring_words(n)}) == 4 ** (n + 2)


def test_the_ring_words_reach_every_case_of_gram_push():
    reached = {}
    for n in (2, 3, 4):
        for lens, _ in S.ring_words(n):
            for case in S.ring_replay(lens, n):
                reached.setdefault(case, (n, lens))
    assert set(reached) == S.RING_CASES, S.RING_CASES ^ set(reached)
    assert len(S.RING_CASES) == 4 + 13 + 3 + 3
    assert S.ring_replay((4, 4, 4, 4), 4) >= {("window16",), ("hi",), ("fill", 12)}
    assert S.ring_replay((3, 3, 3), 4) >= {("straddle", 6)} and S.ring_replay((1, 4, 4), 4) >= {("straddle", 5)}


def test_the_lowered_words_change_length_in_the_ring():
    assert [len(S.utf8(c)) for c in S.LOWERED] == [2, 3, 3, 2] and [len(S.utf8(S.lower(c))) for c in S.LOWERED] == [3, 2, 1, 1]
    assert len(S.lowered_words(3)) == 5 ** 5 and len(S.lowered_words(4)) == (5 ** 6 + 6) // 7
    for n, name in ((3, "tri_default"), (4, "four_nosep_lower")):
        spec = S.SPECS[name][0]
        reached = set()
        for cps in S.lowered_words(n):
            reached |= S.ring_replay([len(S.utf8(S.lower(c))) for c in cps], n)
            assert all(t == t.lower() or "İ" in t for t in S.word_tokens(cps, spec))
        assert {("drop", 1), ("drop", 2), ("drop", 3), ("lo",)} <= reached
        assert any(("straddle", t) in reached for t in (6, 7))


# ---------------- family D ----------------
def test_the_consumer_rows_have_the_verdicts_of_the_restatement_and_the_host():
    rows = S.substring_rows()
    assert len(rows) == 2 * len(S.consumer_code_points()) and len(S.consumer_code_points()) >= 25 + 14
    for tok in (None, SR.TRIGRAM):
        for r, hit, miss in rows:
            assert hit != miss and hit == SR.fold(hit, SR.spec_of(tok)).decode()
            for needle, want in ((hit, True), (miss, False)):
                for e in (Q.Substring(needle), Q.FieldSubstring("t", needle)):
                    assert SR.row_verdict(r.row, e, tok) == want, (r.name, needle)
                    assert Hst.match_row_substring(e, r.row, tok) == want, (r.name, needle)
    assert sorted(Counter(len(S.utf8(c)) for c in S.REGEX_CODE_POINTS).items()) == [(2, 3), (3, 3), (4, 2)]
    for cp in S.REGEX_CODE_POINTS:
        assert S.lower(cp) != cp
        row = S.make_row(b"ab" + S.utf8(cp) + b"cd", (), "", b"t").row
        assert Hst.match_row_regex(Q.FieldRegex("t", "b" + chr(cp) + "c"), row) and not Hst.match_row_regex(Q.FieldRegex("t", "b" + chr(S.lower(cp)) + "c"), row)
        assert TR.row_verdict(row, S.DEFAULT, None, Q.FieldRegex("t", "b" + chr(cp) + "c"))


# ---------------- family E ----------------
def test_keys_are_copied_and_never_lowered():
    for row, hit, miss in S.key_rows():
        assert hit != miss
        assert Hst.match_row(Q.Field(hit), row) and not Hst.match_row(Q.Field(miss), row)
        assert TR.row_verdict(row, S.DEFAULT, Q.Field(hit)) and not TR.row_verdict(row, S.DEFAULT, Q.Field(miss))
    for row, longest, field in S.key_cap_rows():
        assert len(field.encode()) == longest
        assert Hst.match_row(Q.Field(field), row) and TR.row_verdict(row, S.DEFAULT, Q.Field(field))


# ---------------- family F ----------------
def test_the_fault_rows_are_what_they_claim_and_the_host_writes_fffd():
    faults = S.fault_rows()
    assert len({f.row for f in faults}) == len(faults)
    for f in faults:
        if f.documented_only:
            with pytest.raises(ValueError):
                json.loads(f.row.decode())
            continue
        text = S.fault_text(f.row)
        raw_ok = True
        try:
            f.row.decode("utf-8", "strict")
        except UnicodeDecodeError:
            raw_ok = False
        lone = "�" in TR._go_text(json.loads(f.row.decode("utf-8", "replace"))["v"]) if raw_ok else True
        assert f.handed_back == (not raw_ok or lone), f.name                  # handed back exactly when Go would write U+FFFD
        if not f.handed_back:                                     # ... and for no other reason: no unknown code point
            assert not any(S.is_unknown(ord(c)) for c in text.decode("utf-8")), f.name
        want = {t.decode("utf-8") for t in TR.tokens(text, S.DEFAULT)}
        assert any("�" in t for t in want) == f.handed_back, f.name
        es = Hst.EntrySets()
        es.index_row(f.row)
        assert es.as_python_sets() == ({"v"}, want, {"v::" + t for t in want}), f.name
    good = {f.name for f in faults if not f.handed_back}
    assert {"second byte E0 A0", "second byte ED 9F", "second byte F0 90", "second byte F4 8F", "surrogate \\udbff\\uDfFf"} <= good
