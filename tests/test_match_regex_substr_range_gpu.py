"""bsg_match_rows_regex_substr_range (k_match_rows_regex_substr_range / _tok / _gram): FieldRange, FieldRegex and Substring /
FieldSubstring conditions of one table decided in ONE walk of the rows.  Every expected verdict comes from restatements that never ask
the library (tests/range_text_cases.py: the bloom side from tests/ngram_restatement, the regex side from test_match_regex_gpu's
oracle_row under Python `re`, the substring side from tests/substring_restatement, the range side from tests/range_restatement); the
edge cases also state their bits literally.  A call returns no fallback rows, except in the cases that are about them."""
import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst, query as Q
from bloomsearch_amd.gpu import Context
from tests import range_text_cases as RT
from tests import substring_restatement as SR
from tests import walker_envelope_shapes as WE
from tests.helpers import device_ids
from tests.range_text_cases import AND, OR, T, row, want
from tests.test_match_regex_substr_gpu import AT_SINGLE_CAP, OVER_SINGLE_CAP, counted

pytestmark = pytest.mark.gpu

WALKERS = RT.WALKERS


def run(ctx, rows, regex, sub, rng, tok=None, bloom=None, expect=None):
    hits, fb = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowTextRangeQuery(bloom, regex, sub, rng), tok)
    assert list(fb) == [], "rows handed back: %r" % list(fb)
    w = want(rows, bloom, regex, sub, rng, tok)
    assert np.array_equal(hits, w), (np.flatnonzero(hits != w)[:8], [rows[i] for i in np.flatnonzero(hits != w)[:4]])
    if expect is not None:
        assert hits.tolist() == [bool(e) for e in expect]
    return hits


def unsupported(fn, *args, code=_lib.BSG_E_UNSUPPORTED):
    with pytest.raises(_lib.BloomGpuError) as e:
        fn(*args)
    assert e.value.code == code, e.value
    return str(e.value)


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_and_workgroup_edges(ctx, walker, n_rows):
    tok = SR.WALKERS[walker]
    rows = [row(id=i, ts=1700000000 + i, msg="upstream timeout after 3 tries" if i % 2 == 0 else "cache warm", peer="10.0.3.%d" % i if i % 3 == 0 else "10.1.3.%d" % i)
            for i in range(n_rows)]
    rng = Q.FieldRange("ts", 1700000000, 1700000000 + n_rows, hi_open=True)
    hits = run(ctx, rows, Q.FieldRegex("msg", "timeout|cache"), Q.Substring("10.0.3."), rng, tok, expect=[i % 3 == 0 for i in range(n_rows)])
    assert hits[0]
    run(ctx, rows, Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3."), Q.FieldRange("ts", 1700000006, None), tok,
        expect=[i % 6 == 0 and i >= 6 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRegex("msg", "timeout|retry"), None, Q.FieldRange("ts", None, 1700000030, hi_open=True), tok, expect=[i % 2 == 0 and i < 30 for i in range(n_rows)])
    run(ctx, rows, None, Q.FieldSubstring("peer", "10.0."), Q.FieldRange("ts", 1700000003, 1700000009), tok, expect=[i % 3 == 0 and 3 <= i <= 9 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRegex("msg", "."), Q.Substring("10."), Q.FieldRange("id", n_rows - 1, n_rows - 1), tok, expect=[i == n_rows - 1 for i in range(n_rows)])


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("edge", range(len(RT.EDGES)), ids=[e[0].split(":")[0].replace(" ", "_")[:48] for e in RT.EDGES])
def test_edges_state_their_bits(ctx, walker, edge):
    """ONE table per case (regex conditions, then needles, then ranges) under each of the case's programs: the bits are the literal
    ones AND what the restatements say of each condition"""
    tok = SR.WALKERS[walker]
    _, rows, rxs, sxs, rgs, progs = RT.EDGES[edge]
    m, sides = RT.table(rxs, sxs, rgs)
    sat = RT.sat_columns(rows, sides, tok)
    for prog, bits in progs:
        m.prog_ops = list(prog)
        hits, fb = ctx.match_rows_regex_substr_range(rows, m, tok)
        assert list(fb) == []
        assert hits.tolist() == [bool(b) for b in bits] == RT.evaluate(prog, sat).tolist(), prog


def host_verdict(r, bloom, regex, sub, rng, tok):
    """the four host matchers together: what decides a row the device hands back"""
    return bool((bloom is None or Hst.match_row(bloom, r, SR.spec_of(tok))) and Hst.match_row_regex(regex, r) and Hst.match_row_substring(sub, r, tok) and
                Hst.match_row_range(rng, r))


def fallback_case(ctx, rows, regex, sub, rng, tok, handed_back, bits):
    hits, fb = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowTextRangeQuery(None, regex, sub, rng), tok)
    assert list(fb) == handed_back and hits.tolist() == [bool(b) for b in bits]
    w = want(rows, None, regex, sub, rng, tok)
    for i in range(len(rows)):
        if i in handed_back:
            assert not hits[i] and host_verdict(rows[i], None, regex, sub, rng, tok) == bool(w[i]), rows[i]
        else:
            assert hits[i] == w[i], rows[i]


@pytest.mark.parametrize("walker", WALKERS)
def test_each_fallback_cause_beside_a_decided_neighbour(ctx, walker):
    tok = SR.WALKERS[walker]
    rx, sx, rg = Q.FieldRegex("m", "timeout"), Q.Substring("timeout"), Q.FieldRange("v", 1000, 1000)
    # an exponent literal on a range field; the same literal on another leaf hands nothing back
    rows = [b'{"v":1e3,"m":"timeout"}', b'{"v":1000,"m":"timeout"}', b'{"w":1e3,"v":1000,"m":"timeout"}', b'{"v":[1,1E+2],"m":"timeout"}', b'{"v":1000.0,"m":"time out"}']
    fallback_case(ctx, rows, rx, sx, rg, tok, [0, 3], [0, 1, 1, 0, 0])
    # five regex conditions on one leaf (a lane holds four)
    five = Q.RegexOr(*[Q.FieldRegex("a", p) for p in ("x", "^x", "x$", "^x$", ".")])
    rows = [b'{"a":"x","v":1000,"m":"timeout"}', b'{"b":"x","v":1000,"m":"timeout"}', b'{"a":"x","v":7,"m":"timeout"}']
    fallback_case(ctx, rows, Q.RegexAnd(rx, Q.RegexOr(five, Q.FieldRegex("b", "x"))), sx, rg, tok, [0, 2], [0, 1, 0])
    # a rune the lower table cannot decide
    u = RT.unassigned_rune()
    rows = [('{"m":"time%sout timeout","v":1000}' % u).encode(), b'{"m":"timeout","v":1000}', ('{"m":"time%sout","v":1000}' % u).encode()]
    fallback_case(ctx, rows, rx, sx, rg, tok, [0, 2], [0, 1, 0])
    # a row outside the walker's envelope
    assert not WE.in_envelope(RT.DEEP17)
    rows = [RT.DEEP17, b'{"m":"timeout","v":1000}', b'{"m":"timeout","v":1001}']
    fallback_case(ctx, rows, rx, sx, rg, tok, [0], [0, 1, 0])


@pytest.mark.parametrize("walker", WALKERS)
def test_a_full_table_sets_every_flag(ctx, walker):
    """64 conditions: 16 tokens, 16 regex conditions, 16 needles of 8 bytes (both needle words full), 16 ranges; condition c under the
    program [TERM c], bit 63 included"""
    tok = SR.WALKERS[walker]
    rows, blooms, regexes, subs, ranges = RT.full_table()
    m, sides = RT.table(regexes, subs, ranges, blooms)
    assert len(m.kinds) == 64 and m.kinds[63] == _lib.KIND_FIELD_RANGE and sum(len(t) for t, k in zip(m.tokens, m.kinds) if k in (4, 5)) == 128
    sat = RT.sat_columns(rows, sides, tok)
    for c in range(64):
        assert 0 < sat[c].sum() < len(rows)
        m.prog_ops = [T(c)]
        hits, fb = ctx.match_rows_regex_substr_range(rows, m, tok)
        assert list(fb) == [] and np.array_equal(hits, sat[c]), c
    m.prog_ops = [T(c) for c in range(64)] + [OR(64)]
    hits, fb = ctx.match_rows_regex_substr_range(rows, m, tok)
    assert list(fb) == [] and hits.all()
    m.prog_ops = [T(0), T(16), T(32), T(48), AND(4)]
    hits, fb = ctx.match_rows_regex_substr_range(rows, m, tok)
    assert list(fb) == [] and np.array_equal(hits, sat[0] & sat[16] & sat[32] & sat[48]) and hits.tolist() == [i == 0 for i in range(48)]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_table_without_one_family_is_the_parent_call(ctx, walker):
    tok = SR.WALKERS[walker]
    rows = [row(id=i, msg=["connection timeout", "cache miss", "Timeout: lock", "fine"][i % 4], lvl=["err", "inf", "err"][i % 3]) for i in range(130)]
    bloom, rx, sx, rg = Q.FieldToken("lvl", "err"), Q.FieldRegex("msg", "timeout|cache"), Q.Substring("timeout"), Q.FieldRange("id", 10, 99)
    # no kind 6: bsg_match_rows_regex_substr's bits
    a, fa = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowSubstringQuery(bloom, rx, sx), tok)
    b, fb = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, rx, sx), tok)
    assert np.array_equal(a, b) and list(fa) == list(fb) == [] and np.array_equal(a, want(rows, bloom, rx, sx, None, tok)) and a.any()
    # only kind 6 beside the bloom kinds: bsg_match_rows_range's bits
    a, fa = ctx.match_rows_regex_substr_range(rows, Q.CompiledRangeQuery(bloom, rg), tok)
    b, fb = ctx.match_rows_range(rows, Q.CompiledRangeQuery(bloom, rg), tok)
    assert np.array_equal(a, b) and list(fa) == list(fb) == [] and np.array_equal(a, want(rows, bloom, None, None, rg, tok)) and a.any()
    # every mix beside a range condition runs the one family: needles only, regex only, both
    for r, s in ((None, sx), (rx, None), (rx, sx)):
        hits = run(ctx, rows, r, s, rg, tok, bloom=bloom)
        assert 0 < hits.sum() < len(rows)
    # the parents still keep the other family out
    unsupported(ctx.match_rows_range, rows, Q.CompiledRowTextRangeQuery(bloom, rx, None, rg), tok)
    unsupported(ctx.match_rows_regex_substr, rows, Q.CompiledRowTextRangeQuery(bloom, rx, sx, rg), tok, code=_lib.BSG_E_INVALID)


def cap_rows(lens):
    n9, n0, last = lens[-1], lens[0], len(lens) - 1
    return [('{"f%d":"%s","z":"needle","n":5}' % (last, ("ab" * 500)[:n9])).encode(), ('{"f%d":"%s","z":"needle","n":5}' % (last, "c" * (n9 - 1))).encode(),
            ('{"f0":"%s","n":5}' % ("0" * n0)).encode(), ('{"f0":"%s","z":"a NEEDLE","n":6}' % ("0" * n0)).encode(), ('{"f%d":"xyz","z":"needle","n":5}' % last).encode()]


@pytest.mark.parametrize("walker", WALKERS)
def test_the_largest_blob_beside_a_range_condition(ctx, walker):
    """40 448 bytes of regex tables fill the workgroup's 80 KiB behind the needle table, with or without a needle in it: the last
    field's leaf is matched through the highest LDS bytes; four bytes more are refused before any launch"""
    tok = SR.WALKERS[walker]
    rows, rg = cap_rows(AT_SINGLE_CAP), Q.FieldRange("n", 5, 5)
    at, over = Q.RegexOr(*counted(AT_SINGLE_CAP)), Q.RegexOr(*counted(OVER_SINGLE_CAP))
    for sx, bits in ((Q.FieldSubstring("z", "needle"), [1, 0, 0, 0, 0]), (None, [1, 0, 1, 0, 0])):
        hits = run(ctx, rows, at, sx, rg, tok, expect=bits)
        before = int(ctx.device_calls().sum())
        assert "LDS" in unsupported(ctx.match_rows_regex_substr_range, rows, Q.CompiledRowTextRangeQuery(None, over, sx, rg), tok)
        assert int(ctx.device_calls().sum()) == before
    # the blob alone is bsg_match_rows_regex's, under its own larger cap
    hits, fb = ctx.match_rows_regex_substr_range(rows, Q.CompiledRowTextRangeQuery(None, over, None, None), tok)
    assert list(fb) == [] and hits.tolist() == [False, False, True, True, False]


def test_chunked_and_two_device_calls(ctx):
    rows = [row(id=i, msg=("x" * 300) + (" upstream timeout" if i % 2 == 0 else " cache warm"), peer="10.0.3.%d" % i if i % 5 == 0 else "10.1.3.%d" % i)
            for i in range(300)]
    assert sum(len(r) for r in rows) > (1 << 16)
    rx, sx, rg = Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3."), Q.FieldRange("id", 100, 250, lo_open=True)
    expect = [i % 10 == 0 and 100 < i <= 250 for i in range(300)]
    run(ctx, rows, rx, sx, rg, SR.TRIGRAM, expect=expect)
    try:
        for chunk in (1 << 16, 70001):
            ctx.set_ingest_chunk(chunk)
            run(ctx, rows, rx, sx, rg, SR.TRIGRAM, expect=expect)
            assert ctx.last_match_ms() > 0
    finally:
        ctx.set_ingest_chunk(0)
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        before = m.device_calls().copy()
        run(m, rows, rx, sx, rg, None, expect=expect)
        assert int((m.device_calls() - before).sum()) == 2
