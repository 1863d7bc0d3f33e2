"""BloomSearchEngine::query_many with regex queries in the batch: under DeviceMatch + DeviceRegex a query whose patterns all lie in
the device's subset is probed and matched with the batch (bsg_match_rows_many_regex) and still equals what query() returns for it
alone - rows in the same order, every BlockStats field but the duration, Errors, FilesConsidered, FilesBloomSkipped; a pattern
outside the subset and a query that alone puts five patterns on one field go the per-query way; with both switches off nothing
changes.  The point of the feature without a clock: the batch spends less than half the device calls of the single queries."""
import pytest

from bloomsearch_amd import query as Q
from tests import tokenizer_restatement as TR
from tests.test_engine_query_many_gpu import build, check, comparable, queries

pytestmark = pytest.mark.gpu


def rx(field, pattern):
    return Q.FieldRegex(field, pattern)


def in_subset_regex_queries():
    """20 (bloom, regex) queries inside the device subset: shared and distinct fields, one (?i), anchors, trees"""
    return [(None, rx("message", "timeout|cache")),
            (Q.FieldToken("level", "error"), rx("message", "timeout|cache")),               # shares its condition with the query before
            (None, rx("service", "^pay")),
            (Q.Token("timeout"), rx("service", "^pay")),
            (None, rx("message", "(?i)LOGIN")),
            (None, rx("level", "^err")),
            (None, rx("level", "^(warn|info)$")),
            (Q.FieldToken("partition", "p3"), rx("user.name", "^j")),
            (None, rx("user", "^(john|bob)$")),                                            # any leaf beneath user
            (None, rx("user.id", "^[0-3]$")),
            (None, rx("only6", "needle-[12]$")),
            (Q.Field("only6"), rx("partition", "^p6$")),
            (None, rx("partition", "^p[0-2]$")),
            (None, rx("id", "^[0-9]{2}$")),
            (None, Q.RegexAnd(rx("message", "retry"), rx("level", "^err"))),
            (None, Q.RegexOr(rx("only6", "needle-[12]$"), Q.RegexAnd(rx("service", "^pay"), rx("message", "disk")))),
            (Q.Or(Q.FieldToken("partition", "p1"), Q.FieldToken("user.id", "5")), rx("message", "retry")),
            (None, rx("nothere", ".")),                                                    # the field guard prunes every block
            (Q.Token("never-there"), rx("message", "retry")),
            (None, Q.RegexAnd(rx("k" * 100, "timeout"), rx("level", "^err")))]             # a path longer than the device keeps


def mixed_batch():
    """~30 queries, two thirds with regex trees"""
    pairs = in_subset_regex_queries()
    extra = [(None, rx("message", "\\bok\\b")),                                            # outside the device subset: query() answers it
             (Q.FieldToken("level", "info"), Q.RegexOr(*[rx("message", p) for p in ("timeout", "retry", "cache", "^ok", "full$")]))]   # 5 patterns on one field
    plain = [(e, None) for e in queries(10)]
    out = []
    for i in range(max(len(pairs), len(plain))):                                           # regex and plain queries interleaved
        out += pairs[2 * i: 2 * i + 2] + plain[i: i + 1]
    out[7:7] = extra[:1]
    out[20:20] = extra[1:]
    assert len(out) == 32 and sum(r is not None for _, r in out) == 22
    return [b for b, _ in out], [r for _, r in out]


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("spec_name", [None, "punct_lower"])
def test_batch_with_regex_queries_equals_single_queries(ctx, device, spec_name):
    cfg = {} if spec_name is None else {"Tokenizer": TR.SPECS[spec_name], "DeviceIngest": device}
    e = build(ctx, DeviceMatch=device, DeviceRegex=device, **cfg)
    try:
        exprs, regexes = mixed_batch()
        n_rows, pruned, partial = check(e, exprs, regexes)
        assert n_rows > 500 and pruned >= 3 and partial >= 2
        got = e.query_many(exprs, regexes)
        by_query = {i: g for i, g in enumerate(got)}
        hits = [len(g["rows"]) for g in got]
        assert sum(1 for i, h in enumerate(hits) if regexes[i] is not None and h > 0) >= 12       # the regex queries do find rows
        i_pay = next(i for i, r in enumerate(regexes) if r == rx("service", "^pay") and exprs[i] is None)
        assert by_query[i_pay]["rows"] and all(r["service"].startswith("pay") for r in by_query[i_pay]["rows"])
        i_long = next(i for i, r in enumerate(regexes) if r is not None and r.get("Children") and r["Children"][0]["Condition"]["Field"] == "k" * 100)
        assert by_query[i_long]["rows"] and all(r["k" * 100] == "timeout" and r["level"] == "error" for r in by_query[i_long]["rows"])   # rows handed back, decided by the host
        # a batch of regex queries only, and of one
        only = [(b, r) for b, r in zip(exprs, regexes) if r is not None]
        assert check(e, [b for b, _ in only], [r for _, r in only])[0] > 300
        assert check(e, [None], [rx("message", "timeout|cache")])[0] > 0
    finally:
        e.close()


def test_more_regex_conditions_than_one_call_holds(ctx):
    """40 distinct patterns, 10 on each of four fields: groups close on the 16-condition limit and on the slot count"""
    e = build(ctx, DeviceMatch=True, DeviceRegex=True)
    try:
        fields = ["message", "level", "service", "user.name"]
        texts = ["timeout", "retry", "cache", "miss", "ok", "disk", "err", "pay", "j", "a"]
        pairs = [(None, rx(fields[i % 4], texts[i // 4] + ("" if i % 3 else "|zzz"))) for i in range(40)]
        assert len(set((r["Condition"]["Field"], r["Condition"]["Pattern"]) for _, r in pairs)) == 40
        assert check(e, [b for b, _ in pairs], [r for _, r in pairs])[0] > 1000
    finally:
        e.close()


def test_batched_regex_queries_spend_fewer_device_calls(ctx):
    e = build(ctx, DeviceMatch=True, DeviceRegex=True)
    try:
        pairs = in_subset_regex_queries()
        exprs, regexes = [b for b, _ in pairs], [r for _, r in pairs]
        assert len(pairs) == 20
        e.query_many(exprs, regexes)                                                       # arenas leased, tables warm: both sides measured alike
        before = ctx.device_calls().sum()
        many = e.query_many(exprs, regexes)
        mid = ctx.device_calls().sum()
        single = [e.query(b, r) for b, r in pairs]
        after = ctx.device_calls().sum()
        assert [comparable(x) for x in many] == [comparable(x) for x in single]
        spent_many, spent_single = int(mid - before), int(after - mid)
        assert spent_single >= 15, spent_single                                            # every query with rows to scan costs a match call of its own
        assert spent_many * 2 < spent_single, (spent_many, spent_single)
    finally:
        e.close()
