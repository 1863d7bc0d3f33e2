"""The table arithmetic of bsg_match_rows_lookup (no GPU): tests/lookup_plan_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/lookup_plan.hpp, compared with brute-force restatements written here from the header's contract: a string is
found iff it is in the table (whatever shares its slot or its tag), a (field id, token id) pair resolves to its FieldToken condition
and nothing else resolves, a string's record carries every role the table gives it, and the flags are ceil(n_conds / 64) words per
row, word-major over the part's rows."""
import os
import subprocess

import numpy as np
import pytest

from tests.lookup_shapes import want_plan                  # build_strings restated: the lookup shapes place their tables with it too
from tests.test_match_wide_rows_plan import Answers, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_STRING, NO_COND, SLOT_EMPTY = 0xFFFFFFFF, 0xFFFF, 0xFFFFFFFF
FIELD, TOKEN, FIELD_TOKEN = 0, 1, 2
OK, TOO_MANY, KIND = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lookup_plan") / "lookup_plan_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "lookup_plan_check.cpp")],
                   check=True, timeout=300)
    return exe


# ---- the contract, restated ----
def want_slots(n):
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def slot0(h0, slots):
    return h0 & (slots - 1)


def tag(h0):
    return (h0 >> 32) & 0xFFFFF


def pair_slot0(fid, tid, slots):
    return (((fid << 16 | tid) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def check_string_table(tab, h0):
    """every string once, under its tag, reachable from its first slot over occupied slots only"""
    slots = len(tab)
    assert slots == want_slots(len(h0))
    where = {}
    for i, s in enumerate(tab):
        if s != SLOT_EMPTY:
            assert (s & 0xFFF) not in where
            where[s & 0xFFF] = i
    assert sorted(where) == list(range(len(h0))) and SLOT_EMPTY in tab
    for sid, i in where.items():
        assert tab[i] >> 12 == tag(h0[sid])
        j = slot0(h0[sid], slots)
        while j != i:
            assert tab[j] != SLOT_EMPTY, sid
            j = (j + 1) % slots


def strings_case(h0, queries):
    return [0, len(h0)] + list(h0) + [len(queries)] + [x for q in queries for x in q]


def test_every_one_of_2048_strings_is_found_and_absent_keys_miss(driver, tmp_path):
    rng = np.random.default_rng(2048)
    h0 = [int(x) for x in rng.integers(0, 1 << 64, size=2048, dtype=np.uint64)]
    for i in range(100, 160):                                                          # sixty strings in ONE slot, ten of them under one tag as well
        h0[i] = (h0[i] & ~0xFFF) | 0x123
    for i in range(100, 110):
        h0[i] = (h0[i] & ~(0xFFFFF << 32)) | (0xABCDE << 32)
    h0[200] = h0[201]                                                                  # two strings with one key: both are found, in id order
    assert len(set(h0)) == 2047
    present = set(h0)
    absent = [int(x) for x in rng.integers(0, 1 << 64, size=500, dtype=np.uint64)]
    absent += [h ^ (1 << 20) for h in h0[:300]]                                        # the slot AND the tag of a present key, another key
    absent += [h ^ (1 << 40) for h in h0[:300]]                                        # its slot, another tag
    absent += [(h & ~0xFFF) | ((h + 1) & 0xFFF) for h in h0[100:160]]                  # the slot behind a long run
    absent = [k for k in absent if k not in present]
    assert any(slot0(k, 4096) == 0x123 and tag(k) == 0xABCDE for k in absent)
    queries = [(h, i) for i, h in enumerate(h0)] + [(k, NO_STRING) for k in absent] + [(h0[200], NO_STRING)]
    a = run_driver(driver, tmp_path, [strings_case(h0, queries)])
    assert a.take() == 4096
    check_string_table(a.take(4096), h0)
    assert a.take(2048) == list(range(2048))
    assert a.take(len(absent)) == [NO_STRING] * len(absent)
    assert a.take() == 200 and a.done()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 100, 1024, 1025])
def test_smaller_string_tables(driver, tmp_path, n):
    rng = np.random.default_rng(n)
    h0 = [int(x) & 0xFFFFFFFF0000000F for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]   # sixteen first slots for all of them
    queries = [(h, i) for i, h in enumerate(h0)] + [(h ^ (1 << 63), NO_STRING) for h in h0] + [(5, NO_STRING)]
    a = run_driver(driver, tmp_path, [strings_case(h0, queries)])
    slots = a.take()
    check_string_table(a.take(slots), h0)
    assert a.take(n) == list(range(n)) and a.take(n + 1) == [NO_STRING] * (n + 1) and a.done()


def table_case(conds, queries):
    return [1, len(conds)] + [x for c in conds for x in c] + [len(queries)] + [x for q in queries for x in q]


def check_table(a, conds, queries):
    recs, string_of, canon, pairs, pair_cond = want_plan(conds)
    assert a.take(2) == [OK, 0]
    assert a.take() == len(recs) and a.take(len(recs)) == recs
    assert a.take(2 * len(conds)) == string_of and a.take(len(conds)) == canon
    assert a.take() == len(pairs) and a.take(3 * len(pairs)) == [x for p in pairs for x in p]
    slots = a.take()
    assert slots == want_slots(len(pairs))
    assert a.take(len(queries)) == [pair_cond.get(q, NO_COND) for q in queries]
    return len(recs), pair_cond, slots


def test_every_pair_of_a_full_table_resolves_and_no_other(driver, tmp_path):
    rng = np.random.default_rng(7)
    conds = [(FIELD_TOKEN, 10000 + c, 20000 + int(rng.integers(0, 700))) for c in range(1024)]   # 1 024 fields, tokens shared among them
    conds[5] = (FIELD_TOKEN, 10004, conds[4][2] + 1)                                   # one field under two tokens
    recs, _, _, pairs, pair_cond = want_plan(conds)
    assert len(pairs) == 1024 and len(recs) > 1024
    queries = [(f, t) for f, t, _ in pairs] + [(t, f) for f, t, _ in pairs]            # every pair, and every pair swapped
    queries += [(int(f), int(t)) for f, t in rng.integers(0, len(recs), size=(3000, 2))]
    taken = {pair_slot0(f, t, 2048) for f, t, _ in pairs}
    same_slot = [(f, t) for f in range(40) for t in range(len(recs)) if (f, t) not in pair_cond and pair_slot0(f, t, 2048) in taken]
    assert len(same_slot) > 1000                                                       # absent pairs that begin at a present pair's slot
    queries += same_slot
    a = run_driver(driver, tmp_path, [table_case(conds, queries)])
    check_table(a, conds, queries)
    assert a.done()


def test_a_small_table_exhaustively_and_one_string_in_all_four_roles(driver, tmp_path):
    conds = [(FIELD, 7, 0), (TOKEN, 0, 7), (FIELD_TOKEN, 7, 8), (FIELD_TOKEN, 9, 7), (FIELD_TOKEN, 7, 7), (FIELD_TOKEN, 7, 10), (TOKEN, 0, 8),
             (FIELD, 9, 0), (FIELD, 7, 123), (TOKEN, 55, 7), (FIELD_TOKEN, 9, 7), (FIELD, 11, 0), (TOKEN, 0, 12)]
    conds += [(FIELD_TOKEN, 30 + i % 5, 40 + i % 7) for i in range(35)]
    n = len(want_plan(conds)[0])
    queries = [(f, t) for f in range(n) for t in range(n)]                             # every pair of ids there is
    a = run_driver(driver, tmp_path, [table_case(conds, queries)])
    pos = a.at
    check_table(a, conds, queries)
    assert a.done()
    a.at = pos + 2
    recs = a.take(a.take())
    seven = recs[0]                                                                    # "7": the first string
    assert (seven & 0xFFFF, seven >> 16 & 0xFFFF, seven >> 32 & 0xFFFF, seven >> 48) == (0, 0, 1, 3)
    string_of = a.take(2 * len(conds))
    canon = a.take(len(conds))
    assert string_of[0] == 0 and string_of[1] == NO_STRING and string_of[2] == NO_STRING and string_of[3] == 0
    assert canon[8] == 0 and canon[9] == 1 and canon[10] == 3 and canon[4] == 4        # repeated conditions share the first one's bit
    only_token = recs[string_of[2 * 6 + 1]]                                            # "8": a Token condition and a FieldToken token, no path role
    assert only_token >> 16 & 0xFFFF == NO_COND and only_token >> 32 & 0xFFFF == 6 and only_token >> 48 == 2


def test_refused_tables(driver, tmp_path):
    a = run_driver(driver, tmp_path, [table_case([(TOKEN, 0, c) for c in range(1025)], []), table_case([(TOKEN, 0, 1), (FIELD, 2, 0), (3, 4, 5)], []),
                                      table_case([(TOKEN, 0, c) for c in range(1024)], [])])
    assert a.take(2) == [TOO_MANY, 0] and a.take(2) == [KIND, 2] and a.take(3) == [OK, 0, 1024]


@pytest.mark.parametrize("n_conds", [1, 64, 65, 128, 129, 1024])
def test_flag_words_and_offsets(driver, tmp_path, n_conds):
    W = -(-n_conds // 64)
    part_rows, row_base = 1000, 448                                                    # a launch that begins inside the part
    cases = [(n_conds, part_rows, row_base, r, c) for r in (0, 1, 63, 551) for c in sorted({0, n_conds - 1, n_conds // 2, min(63, n_conds - 1), min(64, n_conds - 1)})]
    a = run_driver(driver, tmp_path, [[2] + list(c) for c in cases])
    seen = set()
    for _, _, _, r, c in cases:
        words, index, bit, per_row = a.take(4)
        assert words == W and per_row == 8 * W + 1
        assert index == (c // 64) * part_rows + row_base + r and index < W * part_rows and bit == 1 << (c % 64)
        seen.add((index, bit))
    assert a.done() and len(seen) == len(cases)                                        # no two (row, condition) share a bit
