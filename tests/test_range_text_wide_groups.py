"""The arithmetic of WIDE groups that hold range conditions beside regex and substring ones, on the host (no GPU):
tests/range_text_wide_groups_check.cpp, built with plain g++ against bloomsearch_amd/csrc/host/range_text_groups.hpp — the code the
engine mirror (engine.hpp match_rows_device_many) closes its mixed groups and picks their call by under DeviceMatchRangeTextWide.
References: the rules written out in Python below, and literal answers at each closing rule's edge.  The same driver is built and run
once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: nothing is loaded into python."""
import itertools
import os
import subprocess

import pytest

from tests.test_range_text_groups import FLAGS, ROOT, q, run, token

SRC = os.path.join(ROOT, "tests", "range_text_wide_groups_check.cpp")
WIDE_CAP, WIDE_SUB_CAP = 46592, 42496        # match.hip.h kRxWideLdsCap, kRxWideSubLdsCap
NEW, NEW_ROWS = "bsg_match_rows_wide_regex_substr_range", "bsg_match_rows_wide_regex_substr_range_rows"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("range_text_wide_groups") / "range_text_wide_groups_check"
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", str(exe), SRC], check=True, timeout=600)
    return exe


def fits_line(mix_ok, queries):
    return "F %d " % mix_ok + " ".join(token(x) for x in queries)


def restated(mix_ok, queries):
    """the closing rules of one wide group, written out: per query 1 = it joins (a refused query leaves the group as it was)"""
    has_range = has_text = False
    n_q = n_c = n_rx = rx_bytes = n_needles = 0
    used = [0, 0]
    out = []
    for x in queries:
        r, t = 6 in x["kinds"], any(k in (3, 4, 5) for k in x["kinds"])
        ok = mix_ok or not ((has_range or r) and (has_text or t))
        ok = ok and n_q + 1 <= 1 << 20 and x["query_conds"] <= 64 and n_c + x["conds"] <= 64 and n_rx + x["rx"] <= 16 and x["co_active"] <= 4
        bins = list(used)
        for n in x["needles"]:                                   # first fit, a needle never straddles a word
            w = next((w for w in (0, 1) if 0 < n <= 64 and bins[w] + n <= 64), None)
            if w is None:
                ok = False
                break
            bins[w] += n
        needles = n_needles + len(x["needles"]) != 0
        mixed = (has_range or r) and (has_text or t)
        cap = WIDE_SUB_CAP if (mixed or needles) else WIDE_CAP   # the cap beside the needle table: kind 6 beside a text condition, needle or not
        ok = ok and (rx_bytes + x["rx_bytes"] + 3) // 4 * 4 <= cap
        out.append(int(ok))
        if ok:
            has_range, has_text, used = has_range or r, has_text or t, bins
            n_q, n_c, n_rx, rx_bytes, n_needles = n_q + 1, n_c + x["conds"], n_rx + x["rx"], rx_bytes + x["rx_bytes"], n_needles + len(x["needles"])
    return out


EDGES = [
    # (what, mix_ok, the queries, the literal answer)
    ("the families meet only under the key", 0, [q([6]), q([4], [3])], [1, 0]),
    ("... in either order", 0, [q([3], rx_bytes=100), q([0, 6])], [1, 0]),
    ("with the key they share the group", 1, [q([6]), q([4], [3]), q([3], rx_bytes=100), q([3, 5, 6], [7], 100)], [1, 1, 1, 1]),
    ("no member limit: 70 queries over shared conditions", 1, [q([6])] + [q([4, 6], conds=0, query_conds=2)] * 70, [1] * 71),
    ("64 against 65 conditions", 1, [q([6] * 32), q([4] * 31, [1] * 31), q([5], [1]), q([0])], [1, 1, 1, 0]),
    ("a query of 65 conditions alone, and one of 64", 1, [q([6], conds=1, query_conds=65), q([6], conds=1, query_conds=64)], [0, 1]),
    ("16 against 17 regex conditions", 1, [q([6]), q([3] * 16, rx_bytes=1600), q([3], rx_bytes=100), q([4], [5])], [1, 1, 0, 1]),
    ("co_active_bound 4 against 5: a lane holds four", 1, [q([6]), q([3], rx_bytes=100, co_active=4), q([3], rx_bytes=100, co_active=5)], [1, 1, 0]),
    ("needles at 128 against 129 packed bytes", 1, [q([6]), q([4], [64]), q([5], [64]), q([4], [1])], [1, 1, 1, 0]),
    ("first fit: no word has 30 bytes left", 1, [q([6]), q([4, 4], [40, 40]), q([4], [30]), q([4, 4], [24, 24])], [1, 1, 0, 1]),
    ("a needle over 64 folded bytes", 1, [q([6]), q([4], [65])], [1, 0]),
    ("tables of 42 496 bytes exactly, without a needle", 1, [q([6]), q([3], rx_bytes=WIDE_SUB_CAP)], [1, 1]),
    ("42 500 bytes, without a needle", 1, [q([6]), q([3], rx_bytes=WIDE_SUB_CAP + 4)], [1, 0]),
    ("... and one byte past the cap rounds up to them", 1, [q([6]), q([3], rx_bytes=WIDE_SUB_CAP + 1)], [1, 0]),
    ("42 496 against 42 500 with a needle", 1, [q([4, 6], [8]), q([3], rx_bytes=WIDE_SUB_CAP), q([3], rx_bytes=4)], [1, 1, 0]),
    ("the cap drops when kind 6 arrives", 1, [q([3], rx_bytes=WIDE_SUB_CAP + 4), q([0, 6]), q([0])], [1, 0, 1]),
    ("without kind 6 the wide call's own cap", 1, [q([3], rx_bytes=WIDE_CAP), q([3], rx_bytes=1)], [1, 0]),
    ("with a needle and no kind 6 the cap beside the needle table, as before", 1, [q([3, 4], [3], WIDE_SUB_CAP), q([3], rx_bytes=1)], [1, 0]),
    ("a mixed query alone", 1, [q([3, 4, 6], [8], WIDE_SUB_CAP)], [1]),
    ("... which no group takes without the key", 0, [q([3, 4, 6], [8], 100)], [0]),
]


def test_each_closing_rule_at_its_edge(driver, tmp_path):
    got = run(driver, tmp_path, [fits_line(m, qs) for _, m, qs, _ in EDGES])
    for (what, m, qs, want), g in zip(EDGES, got):
        assert [int(v) for v in g] == want == restated(m, qs), what


def test_random_groups_against_the_rules_written_out(driver, tmp_path):
    import random
    rnd = random.Random(13)
    cases = []
    for _ in range(400):
        qs = []
        for _ in range(rnd.randint(1, 12)):
            kinds = [rnd.choice([0, 1, 2, 3, 4, 5, 6]) for _ in range(rnd.randint(0, 5))]
            needles = [rnd.choice([1, 8, 24, 40, 64, 65]) for k in kinds if k in (4, 5)]
            qs.append(q(kinds, needles, rx_bytes=kinds.count(3) * rnd.choice([100, 9000, 21248, 23296]), conds=rnd.choice([len(kinds), len(kinds) + 20]),
                        co_active=rnd.choice([0, 1, 4, 5])))
        cases.append((rnd.randint(0, 1), qs))
    got = run(driver, tmp_path, [fits_line(m, qs) for m, qs in cases])
    verdicts = set()
    for (m, qs), g in zip(cases, got):
        assert [int(v) for v in g] == restated(m, qs), (m, qs)
        verdicts.update(int(v) for v in g)
    assert verdicts == {0, 1}


def test_mixing_caps_and_the_call_of_a_group(driver, tmp_path):
    lines, want = [], []
    for dm, key, wide_key, wide in itertools.product((0, 1), repeat=4):     # the truth table over all key combinations
        lines.append("M %d %d %d %d" % (dm, key, wide_key, wide))
        want.append([str(int(dm and key and wide_key and wide))])
    for rng, text, needles in itertools.product((0, 1), repeat=3):
        lines.append("C %d %d %d 12345" % (rng, text, needles))
        # a mixed table: 42 496 with and without needles; else the needle table's cap, else the call's own
        want.append([str(WIDE_SUB_CAP if (rng and text) or needles else 12345)])
    names = {(0, 0, 0): "bsg_match_rows_wide", (0, 1, 0): "bsg_match_rows_wide", (0, 0, 1): "bsg_match_rows_wide_substr",
             (0, 1, 1): "bsg_match_rows_wide_substr", (1, 0, 0): "bsg_match_rows_wide_range"}
    for rng, regex, needles, wide_rows in itertools.product((0, 1), repeat=4):
        text = int(regex or needles)
        lines.append("K %d %d %d %d %d" % (rng, text, regex, needles, wide_rows))
        want.append([(NEW_ROWS if wide_rows else NEW) if rng and text else names[(rng, regex, needles)] + ("_rows" if wide_rows else "")])
    assert run(driver, tmp_path, lines) == want


def test_the_driver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "range_text_wide_groups_check_san"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] + FLAGS + ["-o", str(exe), SRC],
                   check=True, timeout=600)
    got = run(exe, tmp_path, [fits_line(m, qs) for _, m, qs, _ in EDGES] + ["M 1 1 1 1", "M 1 1 0 1", "C 1 1 0 7", "K 1 1 1 0 0", "K 1 1 0 1 1"])
    assert [[int(v) for v in g] for g in got[:len(EDGES)]] == [w for _, _, _, w in EDGES]
    assert got[len(EDGES):] == [["1"], ["0"], [str(WIDE_SUB_CAP)], [NEW], [NEW_ROWS]]


def test_the_header_states_the_kernels_cap_and_the_engine_uses_the_wide_rules():
    text = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "host", "range_text_groups.hpp")).read()
    assert "kWideMixedCap = bsh_rxg::kWideSubLdsCap" in text
    groups = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "host", "regex_groups.hpp")).read()
    assert "kWideSubLdsCap = %d;" % WIDE_SUB_CAP in groups
    engine = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "host", "engine.hpp")).read()
    assert "bsh_rtg::wide_mixing(" in engine and "bsh_rtg::wide_regex_table_cap(" in engine and "bsh_rtg::wide_group_call_name(" in engine
