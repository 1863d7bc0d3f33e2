"""bsg_match_rows_substr (k_match_rows_substr / _tok / _gram): Substring and FieldSubstring conditions decided exactly by the device
row walker's shift-and text consumer.  The oracle is the host matcher (bsh_match_row_substring AND bsh_match_row_with); the cases
that pin an edge also state the verdicts they expect.  Every row is inside the device walker's envelope and every call must come
back without fallback rows, except the one case that is about a fallback row."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q
from bloomsearch_amd._lib import OP_TERM, op
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from tests import substring_restatement as SR

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)


def oracle(rows, bloom, sub, tok):
    return np.array([Hst.match_row_substring(sub, r, tok) and (bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) for r in rows], dtype=bool)


def run(ctx, rows, sub, tok=None, bloom=None, expect=None):
    hits, fb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(bloom, sub), tok)
    assert list(fb) == [], "rows handed back: %r" % list(fb)
    want = oracle(rows, bloom, sub, tok)
    assert np.array_equal(hits, want), (np.flatnonzero(hits != want)[:8], [rows[i] for i in np.flatnonzero(hits != want)[:4]])
    if expect is not None:
        assert hits.tolist() == [bool(e) for e in expect]
    return hits


def row(**kv):
    import json
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_and_workgroup_edges(ctx, walker, n_rows):
    rows = [row(id=i, msg="peer %d: Connection reset by peer" % i if i % 3 == 0 else "request %d served" % i, lvl="info") for i in range(n_rows)]
    hits = run(ctx, rows, Q.Substring("ction res"), SR.WALKERS[walker], expect=[i % 3 == 0 for i in range(n_rows)])
    assert hits[0]
    run(ctx, rows, Q.FieldSubstring("id", str(n_rows - 1)), SR.WALKERS[walker])      # a number's raw literal; the last row matches
    run(ctx, rows, Q.Substring("absent"), SR.WALKERS[walker], expect=[False] * n_rows)


@pytest.mark.parametrize("walker", WALKERS)
def test_needle_at_every_position_of_a_24_byte_text_and_every_alignment(ctx, walker):
    """a 3-byte needle at each of the 22 positions of a 24-byte ASCII text (the first and the last byte of the leaf included), the
    leaf itself at each of 9 alignments to the walker's 8-byte scan step (the key grows by a byte); beside each a text that has
    the needle's bytes, but not in its order"""
    rows, expect = [], []
    for shift in range(9):
        key = "t" + "k" * shift
        for p in range(22):
            rows.append(row(**{key: "a" * p + "xyz" + "a" * (21 - p)}))
            expect.append(True)
            rows.append(row(**{key: "z" + "a" * p + "xy" + "a" * (21 - p)}))
            expect.append(False)
    run(ctx, rows, Q.Substring("xyz"), SR.WALKERS[walker], expect=expect)
    run(ctx, rows, Q.SubstringAnd(Q.Substring("XYZ"), Q.Substring("aaaaaaaaaaa")), SR.WALKERS[walker], expect=expect)


@pytest.mark.parametrize("walker", WALKERS)
def test_needles_across_separators_escapes_and_multi_byte_runes(ctx, walker):
    tok = SR.WALKERS[walker]
    rows = [b'{"t":"left right"}', b'{"t":"ab\\ncd"}', b'{"t":"ab\\u00e9cd"}', '{"t":"abÉcd"}'.encode(), b'{"t":"ab\\\\cd\\"e"}',
            '{"t":"aKb"}'.encode(), b'{"t":"a\\u212ab"}', '{"t":"x\U0001F600y"}'.encode(), b'{"t":"x\\ud83d\\ude00y"}', b'{"t":"a,b;c"}',
            b'{"t":true,"u":false,"n":1E5,"z":null}']
    run(ctx, rows, Q.Substring("ft ri"), tok, expect=[1] + [0] * 10)
    run(ctx, rows, Q.Substring("b\nc"), tok, expect=[0, 1] + [0] * 9)
    run(ctx, rows, Q.Substring("béc"), tok, expect=[0, 0, 1, 1] + [0] * 7)                # raw and escaped, folded from upper case
    run(ctx, rows, Q.Substring("BÉC"), tok, expect=[0, 0, 1, 1] + [0] * 7)
    run(ctx, rows, Q.Substring("©c"), tok, expect=[0] * 11)                                 # C3 A9 is not C2 A9
    run(ctx, rows, Q.Substring('b\\cd"e'), tok, expect=[0, 0, 0, 0, 1] + [0] * 6)
    run(ctx, rows, Q.Substring("akb"), tok, expect=[0] * 5 + [1, 1] + [0] * 4)                   # U+212A KELVIN SIGN lowers to k
    run(ctx, rows, Q.Substring("AKB"), tok, expect=[0] * 5 + [1, 1] + [0] * 4)
    run(ctx, rows, Q.Substring("x\U0001F600y"), tok, expect=[0] * 7 + [1, 1, 0, 0])
    run(ctx, rows, Q.Substring(",b;"), tok, expect=[0] * 9 + [1, 0])
    run(ctx, rows, Q.Substring("ru"), tok, expect=[0] * 10 + [1])                                # true
    run(ctx, rows, Q.Substring("E5"), tok, expect=[0] * 10 + [1])                                # the raw literal 1E5, folded
    run(ctx, rows, Q.FieldSubstring("u", "ALS"), tok, expect=[0] * 10 + [1])
    run(ctx, rows, Q.Substring("null"), tok, expect=[0] * 11)                                    # null is never a candidate text
    run(ctx, rows, Q.Substring("t"), tok, expect=[1] + [0] * 9 + [1])                            # never a key: "t" only in `left right` and `true`


def test_without_lower_the_test_is_case_sensitive(ctx):
    rows = [b'{"t":"Hello World"}', b'{"t":"hello world"}', '{"t":"Été"}'.encode()]
    run(ctx, rows, Q.Substring("Hello"), SR.RAW, expect=[1, 0, 0])
    run(ctx, rows, Q.Substring("hello"), SR.RAW, expect=[0, 1, 0])
    run(ctx, rows, Q.Substring("Ét"), SR.RAW, expect=[0, 0, 1])
    run(ctx, rows, Q.Substring("ét"), SR.RAW, expect=[0, 0, 0])
    run(ctx, rows, Q.Substring("hello"), None, expect=[1, 1, 0])


@pytest.mark.parametrize("walker", WALKERS)
def test_nothing_is_carried_from_one_leaf_to_the_next(ctx, walker):
    rows = [b'{"a":"con","b":"nect"}', b'{"a":["con","nect"]}', b'{"a":"connect"}', b'{"a":["x","connect"]}', b'{"a":"con","b":null,"c":"nect"}',
            b'{"a":{"b":"con"},"c":"nect"}']
    run(ctx, rows, Q.Substring("connect"), SR.WALKERS[walker], expect=[0, 0, 1, 1, 0, 0])
    run(ctx, rows, Q.FieldSubstring("a", "connect"), SR.WALKERS[walker], expect=[0, 0, 1, 1, 0, 0])


def term_programs(ctx, rows, needles, tok=None):
    """the verdict of EACH condition of one table (so one packing): the same table under the programs TERM 0, TERM 1, ..."""
    m = Q.CompiledSubstringQuery(None, Q.SubstringOr(*needles))
    out = []
    for c in range(len(needles)):
        m.prog_ops = [op(OP_TERM, c)]
        hits, fb = ctx.match_rows_substr(rows, m, tok)
        assert list(fb) == []
        assert np.array_equal(hits, oracle(rows, None, needles[c], tok))
        out.append(hits.tolist())
    return out


def test_nothing_is_carried_from_one_packed_needle_to_the_next(ctx):
    rows = [b'{"t":"abd"}', b'{"t":"abcd"}', b'{"t":"add"}']
    got = term_programs(ctx, rows, [Q.Substring("ab"), Q.Substring("bc"), Q.Substring("dd")])
    assert got == [[True, True, False], [False, True, False], [False, False, True]]


def test_two_needles_in_different_words(ctx):
    n1, n2 = "".join(chr(97 + i % 26) for i in range(60)), "".join(chr(48 + i % 10) for i in range(60))
    rows = [row(t="<" + n1 + ">"), row(t="<" + n2 + ">"), row(t=n1[:59] + "!" + n2[1:]), row(t=n1, u=n2)]
    got = term_programs(ctx, rows, [Q.Substring(n1), Q.Substring(n2), Q.FieldSubstring("u", "789")])
    assert got == [[True, False, False, True], [False, True, False, True], [False, False, False, True]]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_field_condition_sees_the_leaves_of_its_own_path_only(ctx, walker):
    rows = [b'{"a":{"b":"the needle","c":"hay"}}', b'{"a":{"b":"hay","c":"the needle"}}', b'{"a":"the needle"}', b'{"a":{"b":{"d":"the needle"}}}',
            b'{"a":{"b":["hay","needle"]}}', b'{"a.b":"needle"}']
    tok = SR.WALKERS[walker]
    run(ctx, rows, Q.FieldSubstring("a.b", "needle"), tok, expect=[1, 0, 0, 0, 1, 1])
    run(ctx, rows, Q.FieldSubstring("a", "needle"), tok, expect=[0, 0, 1, 0, 0, 0])               # not the leaf a.b: no prefix rule
    run(ctx, rows, Q.FieldSubstring("a.c", "needle"), tok, expect=[0, 1, 0, 0, 0, 0])
    run(ctx, rows, Q.SubstringAnd(Q.FieldSubstring("a.b", "hay"), Q.FieldSubstring("a.c", "needle")), tok, expect=[0, 1, 0, 0, 0, 0])


@pytest.mark.parametrize("walker", WALKERS)
def test_a_program_over_all_five_kinds(ctx, walker):
    rng = np.random.default_rng(11)
    msgs = ["connection timeout", "Connection reset by peer", "timeout foo", "all good", "foo bar", "conn refused: TIMEOUT"]
    lvls = ["error", "info", "warn"]
    rows = []
    for i in range(200):
        d = {"msg": msgs[rng.integers(0, len(msgs))], "lvl": lvls[rng.integers(0, 3)]}
        if rng.random() < 0.4:
            d["x"] = int(rng.integers(0, 50))
        if rng.random() < 0.3:
            d["note"] = msgs[rng.integers(0, len(msgs))]
        rows.append(row(**d))
    bloom = Q.Or(Q.And(Q.Field("x"), Q.Token("foo")), Q.FieldToken("lvl", "error"), Q.Token("bar"))
    sub = Q.SubstringOr(Q.SubstringAnd(Q.Substring("imeo"), Q.FieldSubstring("msg", "conn")), Q.FieldSubstring("lvl", "RRO"), Q.FieldSubstring("note", "o b"))
    hits = run(ctx, rows, sub, SR.WALKERS[walker], bloom=bloom)
    assert 0 < hits.sum() < len(rows)
    assert np.array_equal(hits, np.array([SR.row_verdict(r, sub, SR.WALKERS[walker]) for r in rows]) & oracle(rows, bloom, None, SR.WALKERS[walker]))


def test_the_nil_program_matches_every_row(ctx):
    rows = [b'{"a":1}', b'{"b":"x"}'] * 40
    hits, fb = ctx.match_rows_substr(rows, Q.CompiledMatcher(None))
    assert list(fb) == [] and hits.all()
    hits, fb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(None, None), SR.TRIGRAM)
    assert list(fb) == [] and hits.all()


@pytest.mark.parametrize("walker", ["default", "separators"])
def test_a_rune_the_lower_table_cannot_decide_hands_the_row_back(ctx, walker):
    rows = [b'{"t":"needle one"}', '{"t":"nee\u0378dle needle"}'.encode(), b'{"t":"no"}', '{"t":"the \u00c9 needle"}'.encode()]
    hits, fb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(None, Q.Substring("needle")), SR.WALKERS[walker])
    assert list(fb) == [1] and hits.tolist() == [True, False, False, True]
    assert Hst.match_row_substring(Q.Substring("needle"), rows[1], SR.WALKERS[walker])              # what the host then decides


def test_a_row_set_split_over_two_upload_chunks(ctx):
    rows = [row(id=i, msg=("x" * 300) + (" Reset by peer" if i % 5 == 0 else " fine")) for i in range(300)]
    assert sum(len(r) for r in rows) > (1 << 16)
    try:
        ctx.set_ingest_chunk(1 << 16)
        run(ctx, rows, Q.Substring("x reset"), SR.TRIGRAM, expect=[i % 5 == 0 for i in range(300)])
    finally:
        ctx.set_ingest_chunk(0)
