"""bsg_match_rows_regex_substr (k_match_rows_regex_substr / _tok / _gram): FieldRegex and Substring / FieldSubstring conditions of one
table decided in ONE walk of the rows, every candidate text fed to both consumers.  Every expected verdict comes from restatements
that never ask the library: the bloom side from tests/ngram_restatement.row_verdict, the regex side from test_match_regex_gpu's
oracle_row under Python `re` (its PY table, and the literal patterns of EXTRA), the substring side from
tests/substring_restatement.row_verdict; the cases that pin an edge also state the bits they expect.  Rows stay inside the device
walker's envelope and a call returns no fallback rows, except in the case that is about them."""
import json
import re

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q
from bloomsearch_amd._lib import OP_AND, OP_OR, OP_TERM, op
from bloomsearch_amd.gpu import Context
from tests import ngram_restatement as NR
from tests import substring_restatement as SR
from tests.helpers import device_ids
from tests.test_match_regex_gpu import PY, oracle_row

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)
# patterns beside test_match_regex_gpu.PY: literals, the same in Python `re`
EXTRA = {p: p for p in ("TIMEOUT", "timeout", "conn", "connect", "timeout|refused")}
SINGLE_CAP, MANY_CAP = 40448, 34032              # match.hip.h kRxSubLdsCap, kRxManySubLdsCap


def py_runner(pattern, text):
    return re.search(PY[pattern] if pattern in PY else EXTRA[pattern], text) is not None


def want(rows, bloom, regex, sub, tok):
    return np.array([NR.row_verdict(r, SR.spec_of(tok), bloom, None) and oracle_row(r, None, regex, py_runner) and SR.row_verdict(r, sub, tok)
                     for r in rows], dtype=bool)


def run(ctx, rows, regex, sub, tok=None, bloom=None, expect=None):
    hits, fb = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, regex, sub), tok)
    assert list(fb) == [], "rows handed back: %r" % list(fb)
    w = want(rows, bloom, regex, sub, tok)
    assert np.array_equal(hits, w), (np.flatnonzero(hits != w)[:8], [rows[i] for i in np.flatnonzero(hits != w)[:4]])
    if expect is not None:
        assert hits.tolist() == [bool(e) for e in expect]
    return hits


def table_programs(ctx, rows, regexes, subs, programs, tok=None):
    """ONE table (the regex conditions first, then the substring ones: one blob, one packing) under each of `programs`; the
    conditions' own verdicts come from the restatements -> [bits of program p]"""
    m = Q.CompiledRowSubstringQuery(None, Q.RegexAnd(*regexes), Q.SubstringAnd(*subs))
    assert len(m.kinds) == len(regexes) + len(subs)
    sat = [want(rows, None, r, None, tok) for r in regexes] + [want(rows, None, None, s, tok) for s in subs]

    def ev(prog):
        stack = []
        for o in prog:
            opc, arg = o >> 28, o & 0x0FFFFFFF
            if opc == OP_TERM:
                stack.append(sat[arg])
            else:
                kids, stack = stack[len(stack) - arg:], stack[:len(stack) - arg]
                stack.append(np.logical_and.reduce(kids) if opc == OP_AND else np.logical_or.reduce(kids))
        return stack[0]
    out = []
    for prog in programs:
        m.prog_ops = list(prog)
        hits, fb = ctx.match_rows_regex_substr(rows, m, tok)
        assert list(fb) == []
        assert np.array_equal(hits, ev(prog)), prog
        out.append(hits.tolist())
    return out


def row(**kv):
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


T = lambda c: op(OP_TERM, c)


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_row_counts_at_the_wave_and_workgroup_edges(ctx, walker, n_rows):
    rows = [row(id=i, msg="upstream timeout after 3 tries" if i % 2 == 0 else "cache warm", peer="10.0.3.%d" % i if i % 3 == 0 else "10.1.3.%d" % i)
            for i in range(n_rows)]
    hits = run(ctx, rows, Q.FieldRegex("msg", "timeout|cache"), Q.Substring("10.0.3."), SR.WALKERS[walker], expect=[i % 3 == 0 for i in range(n_rows)])
    assert hits[0]
    run(ctx, rows, Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3."), SR.WALKERS[walker], expect=[i % 6 == 0 for i in range(n_rows)])
    run(ctx, rows, Q.FieldRegex("msg", "^err"), Q.FieldSubstring("peer", "10."), SR.WALKERS[walker], expect=[False] * n_rows)
    run(ctx, rows, Q.FieldRegex("msg", "."), Q.FieldSubstring("id", str(n_rows - 1)), SR.WALKERS[walker])      # the last row matches


@pytest.mark.parametrize("walker", WALKERS)
def test_one_leaf_feeds_the_two_consumers_differently(ctx, walker):
    """the DFAs read the raw bytes, the needles the folded ones"""
    rows = [b'{"t":"Request TIMEOUT"}']
    tok = SR.WALKERS[walker]
    got = table_programs(ctx, rows, [Q.FieldRegex("t", "TIMEOUT"), Q.FieldRegex("t", "timeout")], [Q.Substring("timeout")],
                         [[T(0)], [T(1)], [T(2)], [T(0), T(2), op(OP_AND, 2)], [T(1), T(2), op(OP_AND, 2)]], tok)
    assert got == [[True], [False], [True], [True], [False]]


def test_without_lower_both_consumers_read_the_raw_bytes(ctx):
    rows = [b'{"t":"Request TIMEOUT"}']
    got = table_programs(ctx, rows, [Q.FieldRegex("t", "TIMEOUT"), Q.FieldRegex("t", "timeout")], [Q.Substring("timeout"), Q.Substring("TIMEOUT")],
                         [[T(0)], [T(1)], [T(2)], [T(3)]], SR.RAW)
    assert got == [[True], [False], [False], [True]]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_regex_field_covers_the_leaves_beneath_it_a_substring_field_its_own_path(ctx, walker):
    rows = [b'{"a":{"b":"connect"}}']
    got = table_programs(ctx, rows, [Q.FieldRegex("a", "conn")], [Q.FieldSubstring("a", "conn"), Q.FieldSubstring("a.b", "conn")],
                         [[T(0)], [T(1)], [T(2)]], SR.WALKERS[walker])
    assert got == [[True], [False], [True]]


@pytest.mark.parametrize("walker", WALKERS)
def test_and_or_and_each_side_alone_over_one_table(ctx, walker):
    # only the regex side, only the substring side, both, neither
    rows = [row(msg="connection timeout", peer="10.1.0.7"), row(msg="all good", peer="10.0.3.9"), row(msg="refused: timeout", note="via 10.0.3.1"),
            row(msg="idle", peer="10.9.9.9")]
    got = table_programs(ctx, rows, [Q.FieldRegex("msg", "timeout|refused")], [Q.Substring("10.0.3.")],
                         [[T(0), T(1), op(OP_AND, 2)], [T(0), T(1), op(OP_OR, 2)], [T(0)], [T(1)]], SR.WALKERS[walker])
    assert got == [[False, False, True, False], [True, True, True, False], [True, False, True, False], [False, True, True, False]]
    run(ctx, rows, Q.FieldRegex("msg", "timeout|refused"), Q.Substring("10.0.3."), SR.WALKERS[walker], bloom=Q.Field("note"), expect=[0, 0, 1, 0])
    run(ctx, rows, Q.FieldRegex("msg", "timeout|refused"), Q.Substring("10.0.3."), SR.WALKERS[walker], bloom=Q.Field("peer"), expect=[0, 0, 0, 0])


@pytest.mark.parametrize("walker", WALKERS)
def test_escapes_and_multi_byte_runes_in_one_leaf(ctx, walker):
    rows = [b'{"t":"ab\\u00e9cd"}', '{"t":"abÉcd"}'.encode(), b'{"t":"\\u212aelvin a\\u212ab"}', '{"t":"日 aKb"}'.encode(), b'{"t":"plain"}']
    got = table_programs(ctx, rows, [Q.FieldRegex("t", "é|日"), Q.FieldRegex("t", "(?i)^k")], [Q.Substring("bé"), Q.Substring("akb")],
                         [[T(0)], [T(1)], [T(2)], [T(3)], [T(0), T(1), T(2), T(3), op(OP_OR, 4)]], SR.WALKERS[walker])
    assert got[0] == [True, False, False, True, False]          # the escape decodes to é; É is another rune to the DFA
    assert got[1] == [False, False, True, False, False]         # U+212A is in the fold orbit of k
    assert got[2] == [True, True, False, False, False]          # ... and É folds to é for the needle
    assert got[3] == [False, False, True, True, False]          # U+212A and K lower to k
    assert got[4] == [True, True, True, True, False]


@pytest.mark.parametrize("walker", WALKERS)
def test_nothing_is_carried_from_one_leaf_to_the_next(ctx, walker):
    rows = [b'{"a":"con","b":"nect"}', b'{"a":["con","nect"]}', b'{"a":"connect"}', b'{"a":["x","connect"]}', b'{"a":"con","b":null,"c":"nect"}',
            b'{"a":{"b":"con"},"c":"nect"}']
    got = table_programs(ctx, rows, [Q.FieldRegex("a", "connect")], [Q.Substring("connect"), Q.FieldSubstring("a", "connect")],
                         [[T(0)], [T(1)], [T(2)], [T(0), T(1), T(2), op(OP_AND, 3)]], SR.WALKERS[walker])
    assert got == [[False, False, True, True, False, False]] * 4


@pytest.mark.parametrize("walker", ["default", "separators"])
def test_fallback_rows_are_the_union_of_the_two_parents(ctx, walker):
    """a leaf under five regex conditions (a lane holds four) and a rune the lower table cannot decide: both rows are handed back
    with their bits 0, the other rows of the same wave are decided"""
    rows = [b'{"a":"x needle"}', b'{"b":"x needle"}', '{"b":"nee\u0378dle needle"}'.encode(), b'{"b":"y"}', b'{"a":"x"}']
    m = Q.CompiledRowSubstringQuery(None, Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^x", "x$", "^x$", ".")]), Q.Substring("needle"))
    assert m.kinds == [_lib.KIND_FIELD_REGEX] * 5 + [_lib.KIND_SUBSTRING]
    for prog, bits in (([T(5)], [0, 1, 0, 0, 0]), ([T(0), T(5), op(OP_OR, 2)], [0, 1, 0, 0, 0]), ([T(0)], [0, 0, 0, 0, 0])):
        m.prog_ops = prog
        hits, fb = ctx.match_rows_regex_substr(rows, m, SR.WALKERS[walker])
        assert list(fb) == [0, 2, 4] and hits.tolist() == [bool(b) for b in bits]
    # four conditions fit a lane: the first and the last row are decided
    m = Q.CompiledRowSubstringQuery(None, Q.RegexAnd(*[Q.FieldRegex("a", p) for p in ("x", "^x", "a", ".")]), Q.Substring("needle"))
    hits, fb = ctx.match_rows_regex_substr(rows, m, SR.WALKERS[walker])
    assert list(fb) == [2] and hits.tolist() == [False] * 5
    m.prog_ops = [T(0), T(1), T(3), op(OP_AND, 3)]
    hits, fb = ctx.match_rows_regex_substr(rows, m, SR.WALKERS[walker])
    assert list(fb) == [2] and hits.tolist() == [True, False, False, False, True]


def counted(lens, first=0):
    return [Q.FieldRegex("f%d" % (first + i), "^[0-9a-f]{%d}$" % n) for i, n in enumerate(lens)]


def unsupported(fn, *args):
    with pytest.raises(_lib.BloomGpuError) as e:
        fn(*args)
    assert e.value.code == _lib.BSG_E_UNSUPPORTED, e.value
    return str(e.value)


# ten counted DFAs: 4 * (sum of the counts) + 2 820 bytes of blob (tests/test_regex_groups.py states the formula): 40 448 exactly, and
# 40 452 with one more state; eight with their user masks: 4 * sum + 2 320 = 34 032 and 34 036
AT_SINGLE_CAP, OVER_SINGLE_CAP = [936 + i for i in range(9)] + [947], [936 + i for i in range(9)] + [948]
AT_MANY_CAP, OVER_MANY_CAP = [987 + i for i in range(7)] + [998], [987 + i for i in range(7)] + [999]


def test_limits_are_refused_before_any_launch(ctx):
    rows = [b'{"a":"x"}']
    single = lambda rx, sx: ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(None, rx, sx))
    many = lambda rx, sx: ctx.match_rows_many_regex_substr(rows, Q.CompiledRowSubstringQueryBatch([(None, rx, sx)]))
    before = int(ctx.device_calls().sum())
    seventeen = Q.RegexOr(*[Q.FieldRegex("a", "x%d" % i) for i in range(17)])
    assert "regex conditions" in unsupported(single, seventeen, Q.Substring("x"))
    batch = Q.CompiledRowSubstringQueryBatch([(None, Q.RegexOr(*seventeen["Children"][:16]), Q.Substring("x"))])
    batch.kinds.append(_lib.KIND_FIELD_REGEX)                   # the seventeenth, past the batch class's own check
    batch.fields.append(b"a")
    batch.tokens.append(b"x16")
    assert "regex conditions" in unsupported(ctx.match_rows_many_regex_substr, rows, batch)
    for call in (single, many):
        assert "needles" in unsupported(call, Q.FieldRegex("a", "x"), Q.SubstringOr(Q.Substring("a" * 40), Q.Substring("b" * 40), Q.Substring("c" * 40)))
        assert "regex condition" in unsupported(call, Q.FieldRegex("a", "\\bx"), Q.Substring("x"))
    # 65 conditions
    unsupported(single, Q.FieldRegex("a", "x"), Q.SubstringOr(*[Q.FieldSubstring("f%d" % i, "x") for i in range(64)]))
    # regex tables the parent call accepts but that do not fit beside the needle table
    assert "LDS" in unsupported(single, Q.RegexOr(*counted(OVER_SINGLE_CAP)), Q.Substring("x"))
    assert "LDS" in unsupported(many, Q.RegexOr(*counted(OVER_MANY_CAP)), Q.Substring("x"))
    assert int(ctx.device_calls().sum()) == before                                      # nothing was launched
    hits, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(None, Q.RegexOr(*counted(OVER_SINGLE_CAP))))
    assert not len(fb) and not hits[0]
    planes, fb = ctx.match_rows_many_regex(rows, Q.CompiledRowQueryBatch([(None, Q.RegexOr(*counted(OVER_MANY_CAP)))]))
    assert not len(fb) and not planes[0][0]
    # ... and without a substring condition the table is the parent call's, with its cap
    hits, fb = single(Q.RegexOr(*counted(OVER_SINGLE_CAP)), None)
    assert not len(fb) and not hits[0]


def cap_rows(lens):
    n9, n0 = lens[-1], lens[0]
    return [('{"f%d":"%s","z":"needle"}' % (len(lens) - 1, ("ab" * 500)[:n9])).encode(), ('{"f%d":"%s","z":"needle"}' % (len(lens) - 1, "c" * (n9 - 1))).encode(),
            ('{"f0":"%s"}' % ("0" * n0)).encode(), ('{"f0":"%s","z":"a NEEDLE"}' % ("0" * n0)).encode(), ('{"f%d":"xyz","z":"needle"}' % (len(lens) - 1)).encode()]


@pytest.mark.parametrize("walker", WALKERS)
def test_tables_that_fill_the_cap_beside_a_needle_table(ctx, walker):
    """the blob takes every byte the needle table leaves of the 80 KiB: the last region and the field strings sit in the highest LDS
    bytes of the workgroup, and the last field's leaf is matched through them"""
    tok = SR.WALKERS[walker]
    rows = cap_rows(AT_SINGLE_CAP)
    m = Q.CompiledRowSubstringQuery(None, Q.RegexOr(*counted(AT_SINGLE_CAP)), Q.FieldSubstring("z", "needle"))
    hits, fb = ctx.match_rows_regex_substr(rows, m, tok)
    assert list(fb) == [] and hits.tolist() == [True, False, False, True, False]
    m.prog_ops = [T(len(AT_SINGLE_CAP) - 1)]
    assert ctx.match_rows_regex_substr(rows, m, tok)[0].tolist() == [True, False, False, False, False]
    rows = cap_rows(AT_MANY_CAP)
    batch = Q.CompiledRowSubstringQueryBatch([(None, Q.RegexOr(*counted(AT_MANY_CAP)), Q.FieldSubstring("z", "needle")),
                                              (None, counted(AT_MANY_CAP)[-1], None), (None, None, Q.FieldSubstring("z", "needle"))])
    planes, fb = ctx.match_rows_many_regex_substr(rows, batch, tokenizer=tok)
    assert list(fb) == []
    assert planes.tolist() == [[True, False, False, True, False], [True, False, False, False, False], [True, True, False, True, True]]


@pytest.mark.parametrize("walker", WALKERS)
def test_a_one_sided_table_is_the_parent_call(ctx, walker):
    tok = SR.WALKERS[walker]
    rows = [row(id=i, msg=["connection timeout", "cache miss", "Timeout: lock", "fine"][i % 4], lvl=["err", "inf", "err"][i % 3]) for i in range(130)]
    bloom, rx, sx = Q.FieldToken("lvl", "err"), Q.FieldRegex("msg", "timeout|cache"), Q.Substring("timeout")
    a, fa = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, rx, None), tok)
    b, fb = ctx.match_rows_regex(rows, Q.CompiledRowQuery(bloom, rx), tok)
    assert np.array_equal(a, b) and list(fa) == list(fb) == [] and np.array_equal(a, want(rows, bloom, rx, None, tok)) and a.any()
    a, fa = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, None, sx), tok)
    b, fb = ctx.match_rows_substr(rows, Q.CompiledSubstringQuery(bloom, sx), tok)
    assert np.array_equal(a, b) and list(fa) == list(fb) == [] and np.array_equal(a, want(rows, bloom, None, sx, tok)) and a.any()
    a, fa = ctx.match_rows_regex_substr(rows, Q.CompiledRowSubstringQuery(bloom, None, None), tok)
    b, fb = ctx.match_rows(rows, Q.CompiledMatcher(bloom), tok)
    assert np.array_equal(a, b) and list(fa) == list(fb) == [] and np.array_equal(a, want(rows, bloom, None, None, tok)) and a.any()
    # the substring pair still keeps regex conditions out
    unsupported(ctx.match_rows_substr, rows, Q.CompiledRowSubstringQuery(bloom, rx, sx), tok)


def test_chunked_and_two_device_calls(ctx):
    rows = [row(id=i, msg=("x" * 300) + (" upstream timeout" if i % 2 == 0 else " cache warm"), peer="10.0.3.%d" % i if i % 5 == 0 else "10.1.3.%d" % i)
            for i in range(300)]
    assert sum(len(r) for r in rows) > (1 << 16)
    rx, sx = Q.FieldRegex("msg", "timeout|retry"), Q.Substring("10.0.3.")
    expect = [i % 10 == 0 for i in range(300)]
    run(ctx, rows, rx, sx, SR.TRIGRAM, expect=expect)
    try:
        for chunk in (1 << 16, 70001):
            ctx.set_ingest_chunk(chunk)
            run(ctx, rows, rx, sx, SR.TRIGRAM, expect=expect)
            assert ctx.last_match_ms() > 0
    finally:
        ctx.set_ingest_chunk(0)
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        before = m.device_calls().copy()
        run(m, rows, rx, sx, None, expect=expect)
        assert int((m.device_calls() - before).sum()) == 2
