"""tests/lookup_shapes.py kept honest (no GPU): its restatement of the table arithmetic against the library's own header, slot for slot,
through tests/lookup_plan_check.cpp fed the cases' REAL h0 values and condition lists; every family's stated property in the model;
coverage of every named edge, computed from the model's touch reports; the model's verdict on every row of every case against the
oracle walker's matcher (tests/tokenizer_restatement.py and tests/ngram_restatement.py under the two specs) — which is what the GPU
test expects of the device; and twelve deliberately wrong rules, each of which changes a verdict, a handed-back list or reads a record
no string has on the case named beside it."""
import numpy as np
import pytest

from tests import lookup_shapes as LS
from tests.test_match_lookup_plan import NO_COND, NO_STRING, driver, strings_case       # noqa: F401 (driver: the fixture)
from tests.test_match_wide_rows_plan import run_driver

CASES = sorted(LS.CASES)


def numbered_conds(case):
    """the case's conditions as lookup_plan_check.cpp reads them: a string is a number's decimal text, equal strings equal numbers"""
    number = {}
    return [(k, number.setdefault(f, len(number) + 1) if k != LS.TOKEN else 0, number.setdefault(t, len(number) + 1) if k != LS.FIELD else 0)
            for k, f, t in case.conds]


def test_the_restated_placement_is_the_headers_slot_for_slot(driver, tmp_path):
    inputs = []
    for name in CASES:
        tab = LS.table_of(name)
        h0 = [h[0] for h in tab.hashes]
        conds = numbered_conds(LS.CASES[name])
        queries = [(f, t) for f, t, _ in tab.pairs] + [(t, f) for f, t, _ in tab.pairs]
        inputs.append(strings_case(h0, [(h, i) for i, h in enumerate(h0)]))
        inputs.append([1, len(conds)] + [x for c in conds for x in c] + [len(queries)] + [x for q in queries for x in q])
        inputs.append([3, len(tab.pairs)] + [x for p in tab.pairs for x in p])
    a = run_driver(driver, tmp_path, inputs)
    sizes = set()
    for name in CASES:
        tab = LS.table_of(name)
        n, n_conds = len(tab.strings), len(tab.conds)
        slots = a.take()
        assert slots == len(tab.str_slots) == LS.table_slots(n), name
        assert a.take(slots) == tab.str_slots, name                                    # the string table, slot for slot
        assert a.take(n) == list(range(n)), name                                       # find_string finds every string under its own h0
        assert a.take(2) == [0, 0] and a.take() == n and a.take(n) == tab.recs, name   # build_strings: records, ...
        assert a.take(2 * n_conds) == tab.string_of and a.take(n_conds) == tab.canon, name
        assert a.take() == len(tab.pairs) and a.take(3 * len(tab.pairs)) == [x for p in tab.pairs for x in p], name
        assert a.take() == len(tab.pair_slots), name
        assert a.take(2 * len(tab.pairs)) == [c for _, _, c in tab.pairs] + [tab.pair_cond.get((t, f), NO_COND) for f, t, _ in tab.pairs], name
        slots = a.take()
        assert slots == len(tab.pair_slots) == LS.table_slots(len(tab.pairs)), name
        assert a.take(slots) == tab.pair_slots, name                                   # the pair table, slot for slot
        sizes.add((len(tab.str_slots), len(tab.pair_slots)))
    assert a.done()
    assert {s for s, _ in sizes} >= {2, 4, 8, 16, 4096} and {p for _, p in sizes} >= {2, 4, 16, 2048}
    assert NO_STRING == LS.NO_STRING and NO_COND == LS.NO_COND


def test_every_family_is_built_and_its_property_holds():
    LS._assert_properties()                                                            # as at import: every family's docstring, in the model
    built = {}
    for c in LS.CASES.values():
        built.setdefault(c.family, set()).update(c.walkers)
    assert tuple(f for f in LS.FAMILIES if f in built) == LS.FAMILIES and set(built) == set(LS.FAMILIES)
    for f in LS.FAMILIES:
        assert {"default", "separator"} <= built[f], f
        assert ("trigram" in built[f]) == (f in LS.TRIGRAM_FAMILIES), f
    for c in LS.CASES.values():
        assert c.why and len(c.rows) <= 40 and len(c.conds) <= LS.MAX_CONDS, c.name
    assert LS.SEARCHED[0] < 4 * LS.TS.SEARCH_BUDGET


def test_every_named_edge_is_touched_by_some_case():
    where = {}
    for name in LS.CASES:
        for e in LS.touched(name):
            where.setdefault(e, name)
    missing = [e for e in LS.EDGES if e not in where]
    assert not missing, missing
    assert len(set(LS.EDGES)) == len(LS.EDGES)
    # ... and where one would look for it
    for edge, family in (("miss-behind-tag-hit", "tag_twin_absent"), ("match-behind-two-tag-hits", "tag_twins_present"), ("tag-0xFFFFF-twin", "tag_extremes"),
                         ("miss-across-wrap", "run_wrap"), ("run-60", "long_run"), ("flag-word-15-bit-63", "long_run"), ("string-id-2047", "long_run"),
                         ("role-filtered-word", "roles_in_one_run"), ("role-filtered-other-bytes", "collision_behind_the_wrap"),
                         ("collision-behind-match", "collision_behind_the_wrap"), ("pair-miss-across-wrap", "pair_runs"), ("pair-slots-2048", "pair_runs"),
                         ("null-leaf-sets-fid", "one_leaf"), ("tables-empty", "empty_table")):
        assert any(edge in LS.touched(n) for n, c in LS.CASES.items() if c.family == family), (edge, family)


@pytest.mark.parametrize("name", CASES)
def test_the_rule_as_written_gives_the_oracles_verdict(name):
    case = LS.CASES[name]
    for walker in case.walkers:
        want = LS.expected(name, walker)
        assert want.shape == (LS.n_queries(case), len(case.rows))
        got = LS.modelled(name, walker)
        assert [r for r, v in enumerate(got) if v.handed_back] == list(case.handed_back), (name, walker)
        for r, v in enumerate(got):
            assert not v.bad_read
            if r in case.handed_back:                                                  # the host decides such a row: the model's flags are not a verdict
                continue
            assert list(v.bits) == list(want[: len(case.conds), r]), (name, walker, r, case.rows[r][:80])
    assert (case.family == "collision_behind_the_wrap") == bool(case.handed_back)
    if case.conds:                                                                     # a case tells rows apart: some condition holds on one row, not on all
        first = LS.expected(name, case.walkers[0])[: len(case.conds)]
        assert first.any() and not first.all(), name


def test_every_wrong_rule_breaks_a_named_case():
    assert [r.name for r in LS.WRONG_RULES] == list(LS.WRONG_RULE_BREAKS)
    for rule in LS.WRONG_RULES:
        assert LS.first_broken(rule) == LS.WRONG_RULE_BREAKS[rule.name], rule.name
    assert LS.first_broken(LS.Rule) is None and LS.first_broken(LS.wrong("as written, again")) is None
    # the two role rules differ from the rule as written only where hashes are equal and bytes are not
    for rule in LS.WRONG_RULES:
        if rule.name in ("skip the role test", "fingerprint before role"):
            assert all(LS.CASES[n].family == "collision_behind_the_wrap" for n in LS.CASES if LS.differs(n, rule)), rule.name


def test_the_searches_return_what_was_asked_by_the_oracles_hash():
    from oracle import oracle as O
    for slots, slot0, tag in ((4, 3, None), (16, 15, None), (4096, 4095, None), (2, 1, 0xFFFFF)):
        for ns in ("qa", "short") if tag is None and slots < 4096 else ("qa",):
            for s in LS.pick(ns, 2, slots, slot0, tag):
                h0 = O.base_hashes(s)[0]
                assert h0 & (slots - 1) == slot0 and (tag is None or (h0 >> 32) & 0xFFFFF == tag)
    for ns, size, slots in (("qb", 2, 4), ("qb", 3, 8), ("short", 2, 4)):
        for g in LS.tag_groups(ns, size, slots, count=2):
            hs = [O.base_hashes(s)[0] for s in g]
            assert len(set(g)) == size and len({(h >> 32) & 0xFFFFF for h in hs}) == 1 and len({h & (slots - 1) for h in hs}) == 1
    blob = LS.short_words()
    assert len({bytes(w) for w in blob}) == 26 ** 3 and int(np.sum((LS.TS.base_hashes_np(blob)[0] & np.uint64(15)) == 15)) == 1149
