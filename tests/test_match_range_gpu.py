"""bsg_match_rows_range (k_match_rows_range / _tok / _gram): FieldRange conditions decided exactly by the device row walker's number
consumer.  The oracle is the host matcher (bsh_match_row_range AND bsh_match_row_with); the cases that pin an edge also state the
verdicts they expect, from tests/range_restatement.py.  Every row is inside the device walker's envelope and every call must come
back without fallback rows, except the cases that are about them."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd._lib import OP_TERM, op
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from tests import range_restatement as RR
from tests import substring_restatement as SR

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)
DOT_DASH = Tokenizer(WHITE_SPACE + ".-", unicode_space=True, lower=True)        # '.' and '-' end a word: the WORDS of -1.5 are 1 and 5


def oracle(rows, bloom, rng, tok):
    return np.array([Hst.match_row_range(rng, r) and (bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) for r in rows], dtype=bool)


def run(ctx, rows, rng, tok=None, bloom=None, expect=None):
    hits, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(bloom, rng), tok)
    assert list(fb) == [], "rows handed back: %r" % list(fb)
    want = oracle(rows, bloom, rng, tok)
    assert np.array_equal(hits, want), (np.flatnonzero(hits != want)[:8], [rows[i] for i in np.flatnonzero(hits != want)[:4]])
    if expect is not None:
        assert hits.tolist() == [bool(e) for e in expect]
    return hits


def row(**kv):
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_and_workgroup_edges(ctx, walker, n_rows):
    tok = SR.WALKERS[walker]
    rows = [row(id=i, lat=i * 0.5, msg="request %d served" % i, lvl="info") for i in range(n_rows)]
    run(ctx, rows, Q.FieldRange("id", 10, 20), tok, expect=[10 <= i <= 20 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRange("id", 10, 20, lo_open=True), tok, expect=[10 < i <= 20 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRange("id", 10, 20, hi_open=True), tok, expect=[10 <= i < 20 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRange("id", 10, 20, lo_open=True, hi_open=True), tok, expect=[10 < i < 20 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRange("lat", 5, 10), tok, expect=[10 <= i <= 20 for i in range(n_rows)])          # 5.0, 5.5, ... 10.0
    run(ctx, rows, Q.FieldRange("id", n_rows - 1, None), tok, expect=[i == n_rows - 1 for i in range(n_rows)])   # only the last row
    run(ctx, rows, Q.FieldRange("msg", None, None), tok, expect=[False] * n_rows)


def term_programs(ctx, rows, conds, tok=None):
    """the verdict of EACH condition of one table: the same table under the programs TERM 0, TERM 1, ..."""
    m = Q.CompiledRangeQuery(None, Q.RangeOr(*conds))
    assert m.kinds == [6] * len(conds)
    out = []
    for c in range(len(conds)):
        m.prog_ops = [op(OP_TERM, c)]
        hits, fb = ctx.match_rows_range(rows, m, tok)
        assert list(fb) == []
        out.append(hits.tolist())
    return out


PAIR_CHUNKS = [RR.BOUND_PAIRS[i: i + 64] for i in range(0, len(RR.BOUND_PAIRS), 64)]
LITERAL_ROWS = [('{"v":%s}' % s).encode() for s in RR.PLAIN_LITERALS]
LITERAL_VALUES = [RR.exact(s) for s in RR.PLAIN_LITERALS]


@pytest.mark.parametrize("chunk", range(len(PAIR_CHUNKS)))
def test_every_plain_literal_against_every_pair_of_bounds(ctx, chunk):
    """one row per literal, up to 64 range conditions on the SAME field in one table: each condition gets its own bit from one parse"""
    pairs = PAIR_CHUNKS[chunk]
    got = term_programs(ctx, LITERAL_ROWS, [RR.field_range(Q, "v", lo, hi) for lo, hi in pairs])
    for c, (lo, hi) in enumerate(pairs):
        want = [RR.inside(v, lo, hi) for v in LITERAL_VALUES]
        assert got[c] == want, (lo, hi, [RR.PLAIN_LITERALS[i] for i in range(len(want)) if got[c][i] != want[i]])
        assert want == [Hst.match_row_range(RR.field_range(Q, "v", lo, hi), r) for r in LITERAL_ROWS]


@pytest.mark.parametrize("walker", WALKERS)
def test_path_and_leaf_rules(ctx, walker):
    tok = SR.WALKERS[walker]
    rows = [r for r, _ in RR.PATH_CASES]
    checks = sorted({(field, bounds) for _, cs in RR.PATH_CASES for field, bounds, _ in cs}, key=repr)
    for field, (lo, hi) in checks:
        hits = run(ctx, rows, RR.field_range(Q, field, lo, hi), tok)
        for i, (_, cs) in enumerate(RR.PATH_CASES):
            for f, b, expected in cs:
                if (f, b) == (field, (lo, hi)):
                    assert bool(hits[i]) == expected, (rows[i], field, lo, hi)


def test_a_number_stays_one_number_under_separators_and_windows(ctx):
    rows = [b'{"v":-1.5}', b'{"v":1.5}', b'{"v":-1}', b'{"v":5}', b'{"v":1}', b'{"v":[-1,5]}', b'{"v":"-1.5"}']
    run(ctx, rows, Q.FieldRange("v", -2, -1, hi_open=True), DOT_DASH, expect=[1, 0, 0, 0, 0, 0, 0])
    run(ctx, rows, Q.FieldRange("v", 1, 2, lo_open=True), DOT_DASH, expect=[0, 1, 0, 0, 0, 0, 0])
    run(ctx, rows, Q.FieldRange("v", 5, 5), DOT_DASH, expect=[0, 0, 0, 1, 0, 1, 0])
    run(ctx, rows, Q.FieldRange("v", -1, -1), DOT_DASH, bloom=Q.FieldToken("v", "1"), expect=[0, 0, 1, 0, 0, 1, 0])
    # the trigram walker raises window requests inside a 12-digit literal
    rows = [b'{"v":123456789012,"w":"abcdefghijkl"}', b'{"v":123456789013}', b'{"v":[1,123456789012.5]}', b'{"v":-123456789012}']
    run(ctx, rows, Q.FieldRange("v", 123456789012, 123456789012), SR.TRIGRAM, expect=[1, 0, 0, 0])
    run(ctx, rows, Q.FieldRange("v", 123456789012, 123456789013, lo_open=True, hi_open=True), SR.TRIGRAM, expect=[0, 0, 1, 0])
    run(ctx, rows, Q.FieldRange("v", None, -123456789012), SR.TRIGRAM, bloom=Q.FieldToken("v", "890"), expect=[0, 0, 0, 1])


@pytest.mark.parametrize("walker", WALKERS)
def test_a_program_over_field_token_fieldtoken_and_fieldrange(ctx, walker):
    tok = SR.WALKERS[walker]
    error, warn = ("err", "war") if walker == "trigram" else ("error", "warn")  # a token of the n-gram walker is a 3-rune window
    rng = np.random.default_rng(5)
    rows = []
    for i in range(200):
        d = {"id": i, "lvl": ["error", "info", "warn"][int(rng.integers(0, 3))], "lat": int(rng.integers(0, 400)) / 2}
        if rng.random() < 0.3:
            d["x"] = int(rng.integers(0, 9))
        if rng.random() < 0.2:
            d["lat"] = [d["lat"], 3]
        rows.append(row(**d))
    h1 = run(ctx, rows, Q.FieldRange("lat", 100, None), tok, bloom=Q.FieldToken("lvl", error))
    h2 = run(ctx, rows, Q.FieldRange("lat", None, 5, hi_open=True), tok, bloom=None)
    assert 0 < h1.sum() < len(rows) and 0 < h2.sum() < len(rows)
    # Or(Field, FieldRange) lives on the bloom side of no tree: the range conditions as terms of one program with the bloom kinds
    m = Q.CompiledRangeQuery(Q.Or(Q.Field("x"), Q.FieldToken("lvl", warn)), Q.FieldRange("lat", None, 5, hi_open=True))
    m.prog_ops[-1] = op(2, 2)                                                    # And(bloom, range) -> Or(bloom, range)
    hits, fb = ctx.match_rows_range(rows, m, tok)
    want = oracle(rows, Q.Or(Q.Field("x"), Q.FieldToken("lvl", warn)), None, tok) | oracle(rows, None, Q.FieldRange("lat", None, 5, hi_open=True), tok)
    assert list(fb) == [] and np.array_equal(hits, want) and 0 < hits.sum() < len(rows)
    # FieldToken and FieldRange on the SAME field share the leaf mask
    both = run(ctx, rows, Q.RangeOr(Q.FieldRange("id", 7, 7), Q.FieldRange("id", 150, None)), tok, bloom=Q.Or(Q.FieldToken("id", "7"), Q.FieldToken("id", "199")))
    assert np.flatnonzero(both).tolist() == [7, 199]
    assert np.array_equal(both, np.array([RR.row_verdict(r, Q.RangeOr(Q.FieldRange("id", 7, 7), Q.FieldRange("id", 199, 199))) for r in rows]))


def test_an_exponent_literal_on_a_range_field_hands_the_row_back(ctx):
    rows = [b'{"v":1000}', b'{"v":1e3}', b'{"v":5,"w":1e3}', b'{"v":[1,1E+21]}', b'{"w":2.5e-7,"v":999}', b'{"v":1000.0}', b'{"v":-1e-400,"u":1}']
    rng = Q.FieldRange("v", 1000, 1000)
    hits, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(None, rng))
    assert list(fb) == [1, 3, 6] and hits.tolist() == [True, False, False, False, False, True, False]
    assert [Hst.match_row_range(rng, rows[i]) for i in fb] == [True, False, False]                      # what the host then decides
    # the same literals on another field: decided on the device
    run(ctx, rows, Q.FieldRange("u", 1, 1), expect=[0, 0, 0, 0, 0, 0, 1])
    # ANY range condition of the table listens, whatever the program reads
    m = Q.CompiledRangeQuery(None, Q.RangeOr(Q.FieldRange("u", 1, 1), Q.FieldRange("w", 0, 1)))
    m.prog_ops = [op(OP_TERM, 0)]
    hits, fb = ctx.match_rows_range(rows, m, SR.TRIGRAM)
    assert list(fb) == [2, 4] and hits.tolist() == [False] * 6 + [True]


def test_a_table_without_a_range_condition_is_the_parent_call(ctx):
    rows = [row(id=i, lvl="err" if i % 3 else "inf", msg="m %d" % i) for i in range(130)]          # words of 3 runes: tokens under every walker
    bloom = Q.And(Q.FieldToken("lvl", "err"), Q.Or(Q.Token("7"), Q.Field("msg")))
    for tok in SR.WALKERS.values():
        a, fa = ctx.match_rows_range(rows, Q.CompiledMatcher(bloom), tok)
        b, fbk = ctx.match_rows(rows, Q.CompiledMatcher(bloom), SR.spec_of(tok))
        assert list(fa) == list(fbk) == [] and np.array_equal(a, b) and 0 < a.sum() < len(rows)
    hits, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(None, None))
    assert list(fb) == [] and hits.all()


def test_a_row_set_split_over_two_upload_chunks(ctx):
    rows = [row(id=i, msg="x" * 300, t=1700000000 + i) for i in range(300)]
    assert sum(len(r) for r in rows) > (1 << 16)
    try:
        ctx.set_ingest_chunk(1 << 16)
        run(ctx, rows, Q.FieldRange("t", 1700000100, 1700000120, hi_open=True), expect=[100 <= i < 120 for i in range(300)])
    finally:
        ctx.set_ingest_chunk(0)
