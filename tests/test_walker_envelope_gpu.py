"""The device row walker (csrc/ingest.hip.h walker_step) at the edges of its envelope — 16 containers, 96 path bytes, one 116-byte LDS
strip per lane — in every kernel family that instantiates it: the ingest walkers and the streaming ingest, the single, batched and
storing row matchers with their regex, substring, regex + substring and range instances, and the lookup walkers, each under the default,
the separator and the n-gram tokenizer.

Every expectation is tests/walker_envelope_shapes.py's: the fallback list is [i for i if not in_envelope(rows[i])] exactly, the bit of
a fallback row is false, every other row is decided as the restatements decide it (tests/ngram_restatement.py,
tests/tokenizer_restatement.py, tests/substring_restatement.py, tests/range_restatement.py), entry sets are the oracle's.  All
comparisons are exact."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, ingest as I, query as Q
from bloomsearch_amd.gpu import pair_rows_list, wide_pair_bits
from oracle import walker_oracle as W
from tests import ngram_restatement as NR
from tests import substring_restatement as SR
from tests import walker_envelope_shapes as S
from tests.test_ingest_gpu import FPR, TRUSTED, check_against_sets

pytestmark = pytest.mark.gpu

WALKERS = sorted(SR.WALKERS)
ROWS = list(S.match_rows())
OUTSIDE = [i for i, r in enumerate(ROWS) if not S.in_envelope(r)]
INSIDE = [i for i, r in enumerate(ROWS) if S.in_envelope(r)]
assert len(ROWS) < 2000 and len(OUTSIDE) > 30 and len(INSIDE) > 60

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def entry_sets_of(walker):
    """the oracle's entry sets of every row, one set per row; computed once and left unchanged"""
    spec = SR.spec_of(SR.WALKERS[walker])
    return cached(("sets", walker), lambda: [NR.entry_sets([r], spec) for r in ROWS])


def wanted(walker, rows_key, rows, qs):
    """bool [len(qs)][len(rows)]: inside the envelope and the restatements' verdict"""
    tok = SR.WALKERS[walker]
    return np.array([cached(("want", walker, rows_key, q.name), lambda q=q: np.array([S.in_envelope(r) and S.reference(r, q, tok) for r in rows], dtype=bool))
                     for q in qs])


# ---------------- ingest ----------------
@pytest.mark.parametrize("flags", [0, TRUSTED], ids=["validated", "trusted"])
@pytest.mark.parametrize("walker", WALKERS)
def test_ingest_one_set_per_row(ctx, walker, flags):
    tok = SR.WALKERS[walker]
    res = I.device_ingest(ctx, [[r] for r in ROWS], FPR, flags=flags, tokenizer=tok)
    assert sorted(int(x) for x in res.fallback_rows) == OUTSIDE, [S.shapes()[i].name for i in set(OUTSIDE) ^ set(int(x) for x in res.fallback_rows) if i < len(S.shapes())]
    assert not res.status.any()
    for i, sets in enumerate(entry_sets_of(walker)):
        check_against_sets(res, i, sets, ROWS[i])


@pytest.mark.parametrize("walker", WALKERS)
def test_a_validating_ingest_has_inserted_nothing_of_a_fallback_row(ctx, walker):
    """the counts BEFORE the host walker's entries are added: nothing for a row outside the envelope, the oracle's for every other"""
    first = np.arange(len(ROWS) + 1, dtype=np.uint32)
    ing = ctx.ingest_rows(ROWS, first, flags=0, tokenizer=SR.WALKERS[walker])
    try:
        assert sorted(int(x) for x in ctx.ingest_fallback_rows(ing)) == OUTSIDE
        counts, status = ctx.ingest_finish(ing, len(ROWS))
    finally:
        ctx.ingest_free(ing)
    assert not status.any()
    want = np.array([[0, 0, 0] if i in set(OUTSIDE) else [len(k) for k in sets] for i, sets in enumerate(entry_sets_of(walker))], dtype=np.uint64)
    assert np.array_equal(counts, want), np.flatnonzero((counts != want).any(axis=1))[:8]


@pytest.mark.parametrize("flags", [0, TRUSTED], ids=["validated", "trusted"])
@pytest.mark.parametrize("walker", WALKERS)
def test_streamed_ingest_of_three_appends(ctx, walker, flags):
    tok = SR.WALKERS[walker]
    cuts = [0, len(ROWS) // 3 + 1, 2 * len(ROWS) // 3 + 2, len(ROWS)]
    with I.IngestStream.open(ctx, len(ROWS), flags=flags, tokenizer=tok) as st:
        for lo, hi in zip(cuts, cuts[1:]):
            fb = st.append(ROWS[lo:hi], list(range(lo, hi)))
            assert [int(x) for x in fb] == [i - lo for i in OUTSIDE if lo <= i < hi], (lo, hi)      # each append returns its own share
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        words = st.build(desc, n_words)
    assert not status.any()
    res = I.IngestResult(counts, status, desc, words, None, None)
    for i, sets in enumerate(entry_sets_of(walker)):
        check_against_sets(res, i, sets, ROWS[i])


def test_ingest_in_64_kib_chunks(ctx):
    copies = 12                                                                 # three chunks, the fallback rows spread over them
    rows = ROWS * copies
    assert sum(len(r) for r in rows) > 2 * (1 << 16) and len(rows) < 2000
    try:
        ctx.set_ingest_chunk(1 << 16)
        res = I.device_ingest(ctx, [[r] for r in rows], FPR)
    finally:
        ctx.set_ingest_chunk(0)
    assert sorted(int(x) for x in res.fallback_rows) == [k * len(ROWS) + i for k in range(copies) for i in OUTSIDE]
    sets = entry_sets_of("default")
    for i in range(len(rows)):
        assert [int(c) for c in res.counts[i]] == [len(k) for k in sets[i % len(ROWS)]], rows[i]
    for i in range((copies - 1) * len(ROWS), len(rows)):                        # the last copy's filters in full
        check_against_sets(res, i, sets[i % len(ROWS)], rows[i])


# ---------------- match ----------------
def _single(method, compiler, parts):
    def run(ctx, rows, qs, tok):
        bits, fbs = [], []
        for q in qs:
            hits, fb = getattr(ctx, method)(rows, compiler(q), tok)
            bits.append(hits)
            fbs.append([int(x) for x in fb])
        return np.array(bits), fbs
    return run, parts


def _many(method, batch_class, item, parts):
    def run(ctx, rows, qs, tok):
        cut = 65                                                                # two sets; the second leaves out query 0
        masks = [(1 << len(qs)) - 1, ((1 << len(qs)) - 1) & ~1]
        planes, fb = getattr(ctx, method)(rows, batch_class([item(q) for q in qs]), [0, cut, len(rows)], masks, tokenizer=tok)
        return np.asarray(planes, dtype=bool), [[int(x) for x in fb]]
    run.masked = lambda want: np.concatenate([want[:1] & (np.arange(want.shape[1]) < 65), want[1:]])
    return run, parts


def _wide(method, batch_class, item, parts, rows_form=False):
    def run(ctx, rows, qs, tok):
        batch = batch_class([item(q) for q in qs])
        if rows_form:
            hdr, pair_off, payload, fb = getattr(ctx, method)(rows, batch, tokenizer=tok)
            bits = np.zeros((len(qs), len(rows)), dtype=bool)
            for p in range(len(qs)):
                bits[p, pair_rows_list(hdr[p], payload[int(pair_off[p]): int(pair_off[p + 1])], len(rows))] = True
        else:
            words, pwo, fb = getattr(ctx, method)(rows, batch, tokenizer=tok)
            bits = np.array([wide_pair_bits(words, pwo, p, len(rows)) for p in range(len(qs))])
        return bits, [[int(x) for x in fb]]
    return run, parts


pair = lambda q: (q.bloom, q.regex)
triple = lambda q: (q.bloom, q.regex, q.substring)
ENTRIES = {
    "match_rows": _single("match_rows", lambda q: Q.CompiledMatcher(q.bloom), ""),
    "match_rows_regex": _single("match_rows_regex", lambda q: Q.CompiledRowQuery(q.bloom, q.regex), "r"),
    "match_rows_substr": _single("match_rows_substr", lambda q: Q.CompiledSubstringQuery(q.bloom, q.substring), "s"),
    "match_rows_regex_substr": _single("match_rows_regex_substr", lambda q: Q.CompiledRowSubstringQuery(q.bloom, q.regex, q.substring), "rs"),
    "match_rows_range": _single("match_rows_range", lambda q: Q.CompiledRangeQuery(q.bloom, q.range), "g"),
    "match_rows_many": _many("match_rows_many", Q.CompiledMatcherBatch, lambda q: q.bloom, ""),
    "match_rows_many_regex": _many("match_rows_many_regex", Q.CompiledRowQueryBatch, pair, "r"),
    "match_rows_many_substr": _many("match_rows_many_substr", Q.CompiledSubstringQueryBatch, lambda q: (q.bloom, q.substring), "s"),
    "match_rows_many_regex_substr": _many("match_rows_many_regex_substr", Q.CompiledRowSubstringQueryBatch, triple, "rs"),
    "match_rows_many_range": _many("match_rows_many_range", Q.CompiledRangeQueryBatch, lambda q: (q.bloom, q.range), "g"),
    "match_rows_wide": _wide("match_rows_wide", Q.CompiledWideBatch, pair, "r"),
    "match_rows_wide_rows": _wide("match_rows_wide_rows", Q.CompiledWideBatch, pair, "r", rows_form=True),
    "match_rows_wide_substr": _wide("match_rows_wide_substr", Q.CompiledWideSubstringBatch, triple, "rs"),
    "match_rows_lookup": _wide("match_rows_lookup", Q.CompiledLookupBatch, pair, ""),
    "match_rows_lookup_rows": _wide("match_rows_lookup_rows", Q.CompiledLookupBatch, pair, "", rows_form=True),
    "match_rows_lookup_regex": _wide("match_rows_lookup_regex", Q.CompiledLookupRegexBatch, pair, "r"),
}


def takes(parts, q):
    return (q.regex is None or "r" in parts) and (q.substring is None or "s" in parts) and (q.range is None or "g" in parts)


def check_entry(ctx, entry, walker, rows_key, rows, qs, outside):
    run, parts = ENTRIES[entry]
    qs = [q for q in qs if takes(parts, q)]
    assert qs
    want = wanted(walker, rows_key, rows, qs)
    inside = np.ones(len(rows), dtype=bool)
    inside[outside] = False
    for i, q in enumerate(qs):                                                  # both verdicts occur among the rows the device decides
        assert want[i][inside].any() and not want[i][inside].all(), q.name
    if hasattr(run, "masked"):
        want = run.masked(want)
    bits, fbs = run(ctx, rows, qs, SR.WALKERS[walker])
    for fb in fbs:
        assert fb == outside, (entry, sorted(set(fb) ^ set(outside))[:8])        # ascending, and exactly the rows outside the envelope
    assert bits.shape == want.shape
    assert not bits[:, outside].any(), entry
    for i, q in enumerate(qs):
        bad = np.flatnonzero(bits[i] != want[i])
        assert len(bad) == 0, (entry, walker, q.name, [rows[j][:60] for j in bad[:4]])


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_match_at_the_envelope(ctx, entry, walker):
    check_entry(ctx, entry, walker, "shapes", ROWS, S.queries(S.token_of(SR.WALKERS[walker])), OUTSIDE)


@pytest.mark.parametrize("family", S.families() + ["alignment"])
def test_match_one_family_alone(ctx, family):
    """a family by itself, from offset 0 of the rows' blob: the alignment rows start where they are designed to"""
    rows = [r for r, _, _ in S.alignment_rows()] if family == "alignment" else [s.row for s in S.shapes() if s.family == family]
    outside = [i for i, r in enumerate(rows) if not S.in_envelope(r)]
    assert outside and len(outside) < len(rows)
    hits, fb = ctx.match_rows(rows, Q.CompiledMatcher(Q.Or(Q.Token("beta"), Q.Token(S.WORD))))
    assert [int(x) for x in fb] == outside
    want = np.array([S.in_envelope(r) and W.matches_bloom_expression(r, Q.Or(Q.Token("beta"), Q.Token(S.WORD))) for r in rows])
    assert np.array_equal(hits, want) and hits.any()


# ---------------- strip isolation ----------------
STRIP_ENTRIES = ["match_rows", "match_rows_regex", "match_rows_substr", "match_rows_regex_substr", "match_rows_lookup_regex"]


@pytest.mark.parametrize("walker", WALKERS)
@pytest.mark.parametrize("entry", STRIP_ENTRIES)
def test_a_full_strip_leaves_its_neighbours_alone(ctx, entry, walker):
    """rows that fill their lane's 116 bytes beside short rows, a full row in the last lane of a workgroup, the first lane of the next
    and the last lane of the launch (behind which the regex blob or the needle table lies): no fallback row, every verdict the reference's"""
    q = S.strip_query(S.token_of(SR.WALKERS[walker]))
    _, parts = ENTRIES[entry]
    q = q._replace(regex=q.regex if "r" in parts else None, substring=q.substring if "s" in parts else None, name="strip_" + parts)
    check_entry(ctx, entry, walker, "strip", list(S.strip_rows()), [q], [])


# ---------------- engine ----------------
def test_an_engine_query_under_device_match_returns_the_oracles_rows(ctx):
    rows = [r for r in ROWS if r.startswith(b"{")]
    assert any(not S.in_envelope(r) for r in rows)
    e = Hst.Engine(ctx, MaxBufferedRows=100000, BloomFalsePositiveRate=1e-4, DeviceMatch=True, DeviceRegex=True)
    try:
        e.ingest_rows(rows)
        e.flush()
        canon = lambda objs: sorted(json.dumps(o, sort_keys=True) for o in objs)
        for bloom, regex in ((Q.Token(S.WORD), None), (Q.Token("beta"), Q.FieldRegex(S.PARENT95, "alpha")), (None, Q.FieldRegex("l" * 97, "alpha"))):
            want = [r for r in rows if S.reference(r, S.Query("engine", bloom, regex, None, None))]
            assert want and any(not S.in_envelope(r) for r in want)             # rows the host finishes are among the answers
            res = e.query(bloom, regex)
            assert res["stats"]["Errors"] == []
            assert canon(res["rows"]) == canon(json.loads(r) for r in want), (bloom, regex)
    finally:
        e.close()
