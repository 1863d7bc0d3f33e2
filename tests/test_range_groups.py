"""The arithmetic of range conditions in a group of batched queries on the host (no GPU): tests/range_groups_check.cpp, built with plain
g++ against bloomsearch_amd/csrc/host/range_groups.hpp — the code the engine mirror (engine.hpp match_rows_device_many) closes its
groups and picks its device calls by.  References: the rule written out in Python (a table never holds kind 6 beside kinds 3-5), the
table of calls, and substring_groups.hpp's own answers for every group without a range condition.  The same driver is built and run
once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: nothing is loaded into python."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "range_groups_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("range_groups") / "range_groups_check"
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", str(exe), SRC], check=True, timeout=600)
    return exe


def run(exe, tmp_path, lines):
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt"), str(tmp_path / "answers.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l.split() for l in (tmp_path / "answers.txt").read_text().splitlines()]
    assert len(out) == len(lines)
    return out


def group_line(queries):
    return "G " + " ".join(",".join(map(str, q)) if q else "-" for q in queries)


def joined(queries):
    """per query: does it join the one group (a refused query leaves the group as it was)"""
    has_range = has_text = False
    verdicts = []
    for q in queries:
        r, t = 6 in q, any(k in (3, 4, 5) for k in q)
        ok = not (r and t) and not ((has_range or r) and (has_text or t))
        verdicts.append(ok)
        if ok:
            has_range, has_text = has_range or r, has_text or t
    return verdicts


def test_a_group_closes_where_kind_6_meets_kinds_3_to_5_in_either_order(driver, tmp_path):
    cases = [
        [[6], [3]], [[6], [4]], [[6], [5]], [[3], [6]], [[4], [6]], [[5], [6]],        # the two families, in either order
        [[0, 6], [1, 2, 5]], [[2, 3], [0, 6]],                                         # ... among a query's other conditions
        [[6], [6, 6], [0, 6]], [[3], [4, 5], [3, 5]],                                   # each family with itself
        [[6], [3], [6]], [[4], [6], [5]],                                               # the refused query left the group as it was
        [[6, 3]],                                                                       # no call takes such a query at all
    ]
    got = run(driver, tmp_path, [group_line(c) for c in cases])
    want = [[1, 0]] * 8 + [[1, 1, 1]] * 2 + [[1, 0, 1]] * 2 + [[0]]
    assert [[int(x) for x in g] for g in got] == want
    assert [[int(v) for v in joined(c)] for c in cases] == want


def test_plain_queries_join_either_side(driver, tmp_path):
    plain = [[], [0], [1], [2], [0, 1, 2]]
    cases = []
    for side in ([6], [3], [4], [5]):
        for p in plain:
            cases += [[side, p, side], [p, side, p], [p, p, side]]
    got = run(driver, tmp_path, [group_line(c) for c in cases])
    assert all(g == ["1", "1", "1"] for g in got)
    # and a plain query between the two families does not reconcile them
    got = run(driver, tmp_path, [group_line([[6], [0], [3]]), group_line([[5], [1, 2], [], [6]])])
    assert got == [["1", "1", "0"], ["1", "1", "1", "0"]]


def test_random_groups_follow_the_rule(driver, tmp_path):
    rng = np.random.default_rng(20261020)
    cases = []
    for _ in range(500):
        pool = [[0, 1, 2, 6], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6]][int(rng.integers(0, 3))]
        cases.append([[int(k) for k in rng.choice(pool, size=int(rng.integers(0, 4)))] for _ in range(int(rng.integers(1, 9)))])
    got = run(driver, tmp_path, [group_line(c) for c in cases])
    want = [joined(c) for c in cases]
    assert [[x == "1" for x in g] for g in got] == want
    assert any(False in w for w in want) and any(all(w) and len(w) > 2 for w in want)


def test_the_call_for_every_combination_of_range_regex_needles_and_the_keys(driver, tmp_path):
    keys = list(itertools.product((0, 1), repeat=5))                 # (range, regex, needles, wide, wide_rows)
    got = [g[0] for g in run(driver, tmp_path, ["K %d %d %d %d %d" % k for k in keys])]
    today = [g[0] for g in run(driver, tmp_path, ["S %d %d %d %d" % k[1:] for k in keys])]
    for k, name, parent in zip(keys, got, today):
        rng, regex, needles, wide, wide_rows = k
        if not rng:
            assert name == parent, k                                 # without a range condition: what substring_groups.hpp answers today
        elif regex or needles:
            assert name == "-", k                                    # no call decides both families: joins() keeps such a group from forming
        else:
            assert name == ("bsg_match_rows_wide_range_rows" if wide_rows else "bsg_match_rows_wide_range" if wide else "bsg_match_rows_many_range"), k
    # the parent's table itself, written out (tests/test_substring_groups.py states the same)
    table = {(0, 0, 0, 0): "bsg_match_rows_many", (1, 0, 0, 0): "bsg_match_rows_many_regex", (0, 1, 0, 0): "bsg_match_rows_many_substr",
             (1, 1, 0, 0): "bsg_match_rows_many_regex_substr", (0, 0, 1, 0): "bsg_match_rows_wide", (1, 0, 1, 0): "bsg_match_rows_wide",
             (0, 1, 1, 0): "bsg_match_rows_wide_substr", (1, 1, 1, 0): "bsg_match_rows_wide_substr", (0, 0, 1, 1): "bsg_match_rows_wide_rows",
             (1, 0, 1, 1): "bsg_match_rows_wide_rows", (0, 1, 1, 1): "bsg_match_rows_wide_substr_rows", (1, 1, 1, 1): "bsg_match_rows_wide_substr_rows",
             (0, 0, 0, 1): "bsg_match_rows_wide_rows", (1, 0, 0, 1): "bsg_match_rows_wide_rows", (0, 1, 0, 1): "bsg_match_rows_wide_substr_rows",
             (1, 1, 0, 1): "bsg_match_rows_wide_substr_rows"}
    for k, name in zip(keys, got):
        if not k[0]:
            assert name == table[k[1:]], k


def test_the_lookup_keys_never_take_a_group_with_a_range_condition(driver, tmp_path):
    keys = list(itertools.product((0, 1), repeat=5))                 # (lookup, lookup_regex, range, regex, needles)
    got = [int(g[0]) for g in run(driver, tmp_path, ["L %d %d %d %d %d" % k for k in keys])]
    for (lookup, lookup_regex, rng, regex, needles), g in zip(keys, got):
        # without a range condition: the rule the engine applied before (a needle never; a regex condition only under the regex key)
        want = bool(lookup and not needles and (not regex or lookup_regex))
        assert g == int(want and not rng), (lookup, lookup_regex, rng, regex, needles)
    assert sum(got) == 3


def test_the_driver_under_the_sanitizers(tmp_path):
    exe = tmp_path / "range_groups_check_asan"
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC], check=True, timeout=600)
    lines = [group_line([[6], [0], [3], [6, 2], [], [4, 5]]), "K 1 0 0 1 1", "K 1 1 0 0 0", "K 0 1 1 0 0", "S 1 1 0 0", "L 1 0 1 0 0", "L 1 1 0 1 0"]
    lines += ["K %d %d %d %d %d" % k for k in itertools.product((0, 1), repeat=5)]
    got = run(exe, tmp_path, lines)
    assert got[:7] == [["1", "1", "0", "1", "1", "0"], ["bsg_match_rows_wide_range_rows"], ["-"], ["bsg_match_rows_many_regex_substr"],
                       ["bsg_match_rows_many_regex_substr"], ["0"], ["1"]]
