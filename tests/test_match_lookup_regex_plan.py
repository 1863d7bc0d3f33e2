"""The plan arithmetic of bsg_match_rows_lookup_regex (no GPU): tests/lookup_regex_plan_check.cpp, built with plain g++ under
-fsanitize=address,undefined against bloomsearch_amd/csrc/host/lookup_plan.hpp and host/regex_groups.hpp, compared with brute-force
restatements written here from the headers' contract: a FieldRegex condition takes no role string and no pair, a repeated one is its
first occurrence, the first occurrences are the regex slots in table order, a set's mask holds the slots its listed queries'
programs reference, and the blob's cap is what the table's strings, pairs and lanes leave of 80 KiB."""
import os
import subprocess

import pytest

from tests.test_match_wide_rows_plan import run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_STRING, NO_COND = 0xFFFFFFFF, 0xFFFF
FIELD, TOKEN, FIELD_TOKEN, REGEX = 0, 1, 2, 3
OK, TOO_MANY, KIND = 0, 1, 2
BLOB_OK, BLOB_TOO_MANY, BLOB_PATTERN, BLOB_OVER_CAP = 0, 1, 2, 3
LANES = 256 * 116
WIDE_CAP = 46592                                                                       # the storing walker's regex cap (match.hip.h kRxWideLdsCap)
TERM, AND, OR = 0, 1, 2


def op(code, arg=0):
    return code << 28 | arg


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lookup_regex_plan") / "lookup_regex_plan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-sign-compare",      # (regex_dfa.hpp compares digits as the library's build does)
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "lookup_regex_plan_check.cpp")], check=True, timeout=300)
    return exe


def string(s):
    b = s if isinstance(s, bytes) else s.encode()
    return [len(b)] + list(b)


def conds_words(conds):
    return [len(conds)] + [x for k, f, t in conds for x in [k] + string(f) + string(t)]


def table_case(conds, programs, set_lists):
    off = [0]
    for l in set_lists:
        off.append(off[-1] + len(l))
    return ([0] + conds_words(conds) + [len(programs)] + [x for p in programs for x in [len(p)] + p] +
            [len(set_lists)] + off + [q for l in set_lists for q in l])


# ---- the contract, restated ----
def slots(n):
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def want_cap(n_strings, n_pairs):
    return 80 * 1024 - (4 * slots(n_strings) + 8 * slots(n_pairs) + LANES)


def want_plan(conds):
    """-> (n_strings, string_of, canon, n_pairs, rx_conds)"""
    ids, string_of, canon, first, pairs, rx_conds = {}, [], [], {}, set(), []

    def sid(s):
        return ids.setdefault(s, len(ids))

    for c, (kind, f, t) in enumerate(conds):
        if kind == REGEX:
            string_of += [NO_STRING, NO_STRING]
            key = (REGEX, f, t)
            if key not in first:
                rx_conds.append(c)
        else:
            fid = sid(f) if kind != TOKEN else NO_STRING
            tid = sid(t) if kind != FIELD else NO_STRING
            string_of += [fid, tid]
            key = (kind, fid, tid)
            if kind == FIELD_TOKEN:
                pairs.add((fid, tid))
        canon.append(first.setdefault(key, c))
    return len(ids), string_of, canon, len(pairs), rx_conds


def want_masks(conds, programs, set_lists):
    _, _, canon, _, rx_conds = want_plan(conds)
    out = []
    for listed in set_lists:
        m = 0
        for q in listed:
            for o in programs[q]:
                if o >> 28 == TERM and canon[o & 0x0FFFFFFF] in rx_conds:
                    m |= 1 << rx_conds.index(canon[o & 0x0FFFFFFF])
        out.append(m)
    return out


def check_table(a, conds, programs, set_lists, plain_status):
    n_strings, string_of, canon, n_pairs, rx_conds = want_plan(conds)
    assert a.take(2) == plain_status                                                   # the plain lookup call's form is as it was
    assert a.take(2) == [OK, 0]
    assert a.take() == n_strings and a.take(2 * len(conds)) == string_of and a.take(len(conds)) == canon
    assert a.take() == n_pairs
    assert a.take() == len(rx_conds) and a.take(len(rx_conds)) == rx_conds
    assert a.take(len(conds)) == [rx_conds.index(canon[c]) if canon[c] in rx_conds else NO_COND for c in range(len(conds))]
    masks = a.take(len(set_lists))
    assert masks == want_masks(conds, programs, set_lists)
    return masks


def test_repeated_regex_conditions_share_the_first_and_take_no_string_and_no_pair(driver, tmp_path):
    conds = [(REGEX, "msg", "^a"), (TOKEN, "", "msg"), (REGEX, "msg", "^a"), (FIELD_TOKEN, "msg", "^a"), (REGEX, "msg", "b$"), (REGEX, "ms", "g^a"),
             (FIELD, "msg", ""), (REGEX, "msg", "b$"), (REGEX, "msg", "^a"), (FIELD_TOKEN, "msg", "^a"), (REGEX, "m", "sg^a")]
    programs = [[op(TERM, c)] for c in range(len(conds))]
    sets = [list(range(len(conds))), [2], [7, 8], [1, 3, 6]]
    a = run_driver(driver, tmp_path, [table_case(conds, programs, sets)])
    masks = check_table(a, conds, programs, sets, [KIND, 0])
    assert a.done()
    _, string_of, canon, n_pairs, rx_conds = want_plan(conds)
    assert rx_conds == [0, 4, 5, 10] and canon == [0, 1, 0, 3, 4, 5, 6, 4, 0, 3, 10]   # the same bytes split otherwise are other conditions
    assert n_pairs == 1 and all(string_of[2 * c] == string_of[2 * c + 1] == NO_STRING for c in (0, 2, 4, 5, 7, 8, 10))
    assert masks == [0b1111, 0b0001, 0b0011, 0]                                        # a repeated condition opens its first occurrence's slot


def test_set_masks_over_a_full_table_with_regex_conditions_in_the_first_and_last_words(driver, tmp_path):
    at = [0, 63, 64, 1023]
    conds = [(REGEX, "r%d" % c, "x|y") if c in at else (TOKEN, "", "t%d" % c) for c in range(1024)]
    programs = [[op(TERM, c)] for c in at]                                             # queries 0-3: each regex condition alone
    programs += [[op(TERM, 5)], [op(TERM, 62), op(TERM, 65), op(OR, 2)], []]           # 4-6: regex-free, the last one the nil expression
    programs += [[op(TERM, 0), op(TERM, 1023), op(AND, 2)], [op(TERM, 1), op(TERM, 64), op(TERM, 1022), op(OR, 3)]]   # 7, 8
    everything = list(range(len(programs)))
    sets = [[], [4, 5, 6], everything, [1, 8], [3], [0, 5]]
    a = run_driver(driver, tmp_path, [table_case(conds, programs, sets), table_case(conds, programs, [everything])])   # ... and the implicit set
    masks = check_table(a, conds, programs, sets, [KIND, 0])
    assert masks == [0, 0, 0b1111, 0b0110, 0b1000, 0b0001]
    assert check_table(a, conds, programs, [everything], [KIND, 0]) == [0b1111]
    assert a.done()


def test_tables_the_regex_form_refuses_or_passes_on(driver, tmp_path):
    many = [(TOKEN, "", "t%d" % c) for c in range(1024)]
    a = run_driver(driver, tmp_path, [table_case(many + [(REGEX, "f", "x")], [], []), table_case([(TOKEN, "", "t"), (4, "a", "b")], [], []),
                                      table_case([(REGEX, "f%d" % i, "x") for i in range(17)], [], []), table_case(many, [], [])])
    assert a.take(4) == [TOO_MANY, 0, TOO_MANY, 0]
    assert a.take(4) == [KIND, 1, KIND, 1]
    conds = [(REGEX, "f%d" % i, "x") for i in range(17)]                               # the 17th is the blob's to refuse: every one is a slot here
    check_table(a, conds, [], [], [KIND, 0])
    check_table(a, many, [], [], [OK, 0])                                              # without a regex condition both forms agree
    assert a.done()


def test_the_cap_at_the_empty_table_and_at_the_limit(driver, tmp_path):
    cases = [(2, 2, 0, 0), (4096, 2048, 2048, 1024), (32, 2, 10, 0), (2, 2, 1, 1), (4, 4, 2, 2), (2048, 1024, 1000, 500)]
    a = run_driver(driver, tmp_path, [[1] + list(c) for c in cases])
    got = [a.take(3) for _ in cases]
    assert a.done()
    assert got[0] == [LANES + 24, 52200, 52200] and got[1] == [62464, 19456, 19456]
    for (ss, ps, ns, np_), (lds, cap, cap_of) in zip(cases, got):
        assert lds == 4 * ss + 8 * ps + LANES and cap == 80 * 1024 - lds and cap_of == want_cap(ns, np_) and lds + cap == 80 * 1024
        assert 19456 <= cap_of <= 52200 < 65536                                        # the blob's 16-bit offsets reach every cap
    assert want_cap(10, 0) == 52080


def blob_case(cap, conds):
    return [2, cap] + conds_words(conds)


def align4(v):
    return (v + 3) & ~3


def estimates_and_size(a):
    est = a.take(a.take())
    return est, a.take()


def test_six_thousand_state_patterns_exceed_a_full_tables_cap_and_fit_a_small_ones(driver, tmp_path):
    pattern, fields = "^[0-9a-f]{1000}$", ["field_%d" % i for i in range(6)]           # 7-byte fields
    six = [(REGEX, f, pattern) for f in fields]
    full = [(FIELD_TOKEN, "f%d" % i, "t%d" % i) for i in range(1008)] + six + [(REGEX, "r%d" % i, "x|y") for i in range(10)]
    small = [(TOKEN, "", "t%d" % i) for i in range(10)] + six
    assert want_plan(full)[0] == 2016 and want_cap(2016, 1008) == 19456 and want_cap(*want_plan(small)[:4:3]) == 52080
    a = run_driver(driver, tmp_path, [[3] + string(pattern) + [7], blob_case(19456, full), blob_case(52080, small), blob_case(WIDE_CAP, small),
                                      blob_case(19456, small[10:13] + full[:1008])])
    assert a.take(4) == [1, 1002, 2, 4287]                                             # 16 + align4(256 + 2 * 1002 * 2) + 7
    assert 6 * 4287 > 19456 and 6 * 4287 <= min(52080, WIDE_CAP)
    assert a.take(4) == [OK, BLOB_OVER_CAP, 0, 16]                                     # over the full table: refused (the estimates stop where it overflowed)
    est, size = estimates_and_size(a)
    assert est == [4287] * len(est) and 4 <= len(est) <= 5 and size == 0
    for _ in range(2):                                                                 # the 10-Token table's cap and the wide call's: accepted
        assert a.take(4) == [OK, BLOB_OK, 0, 6]
        est, size = estimates_and_size(a)
        assert est == [4287] * 6 and align4(6 * 4287) - 4 <= size <= align4(6 * 4287)   # rx_table_bytes' contract: the padded sum, or 4 below
        assert a.take(12) == [x for c in range(10, 16) for x in (c, 7)]                # header word 1 carries the condition of the TABLE
    assert a.take(4) == [OK, BLOB_OK, 0, 3]                                            # three of them fit under the full table
    est, size = estimates_and_size(a)
    assert est == [4287] * 3 and align4(3 * 4287) - 4 <= size <= align4(3 * 4287) <= 19456 and a.take(6) == [0, 7, 1, 7, 2, 7]
    assert a.done()


def test_only_distinct_regex_conditions_count_and_go_into_the_blob(driver, tmp_path):
    others = [(REGEX, "o%d" % i, "x|y") for i in range(15)]
    twenty = [(TOKEN, "", "t")] * 3 + [(REGEX, "message", "a.*b")] * 20
    at_1023 = [(TOKEN, "", "t%d" % i) for i in range(1023)] + [(REGEX, "f", "[0-9]+")]
    a = run_driver(driver, tmp_path, [blob_case(52200, twenty + others), blob_case(52200, twenty + others + [(REGEX, "o15", "x|y")]),
                                      blob_case(52200, [(TOKEN, "", "t"), (REGEX, "a", "\\bx")]), blob_case(19456, at_1023)])
    assert a.take(4) == [OK, BLOB_OK, 0, 16]                                           # 35 regex entries, 16 conditions
    est, size = estimates_and_size(a)
    assert len(est) == 16 and 0 < size <= align4(sum(est)) <= 52200
    assert a.take(32) == [x for c, n in [(3, 7)] + [(23 + i, len("o%d" % i)) for i in range(15)] for x in (c, n)]
    assert a.take(4) == [OK, BLOB_TOO_MANY, 0, 17] and estimates_and_size(a) == ([], 0)   # the 17th distinct one
    assert a.take(4) == [OK, BLOB_PATTERN, 1, 1] and estimates_and_size(a) == ([], 0)  # outside the subset: the condition is named
    assert a.take(4) == [OK, BLOB_OK, 0, 1]
    est, size = estimates_and_size(a)
    assert len(est) == 1 and 0 < size <= 19456
    assert a.take(2) == [1023, 1] and a.done()                                         # the upper 16 bits of header word 1 hold condition 1 023
