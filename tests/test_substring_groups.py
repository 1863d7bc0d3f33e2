"""The arithmetic of substring conditions in a group of batched queries on the host (no GPU): tests/substring_groups_check.cpp, built
with plain g++ against bloomsearch_amd/csrc/host/substring_groups.hpp — the code the engine mirror (engine.hpp
match_rows_device_many) closes its groups and picks its device calls by.  References: a brute-force first-fit in Python over every
prefix of random needle-length sequences (and substring_pack.hpp's own pack_needles over the accepted needles), the stated caps,
and the issue's table of calls."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY_CAP, MANY_SUB_CAP, WIDE_CAP, WIDE_SUB_CAP = 38140, 34032, 46592, 42496      # bloomgpu.h: the regex tables without / beside a needle table


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("substring_groups") / "substring_groups_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare",     # (regex_dfa.hpp compares digits as the library's build does)
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "substring_groups_check.cpp")],
                   check=True, timeout=600)
    return exe


def run(exe, tmp_path, lines):
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt"), str(tmp_path / "answers.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l.split() for l in (tmp_path / "answers.txt").read_text().splitlines()]
    assert len(out) == len(lines)
    return out


def first_fit(lens):
    """per needle: does it find a word (2 words of 64 positions, the first with room; a refused needle leaves the words as they were)"""
    used, verdicts = [0, 0], []
    for n in lens:
        w = next((w for w in range(2) if 0 < n <= 64 and used[w] + n <= 64), None)
        verdicts.append(w is not None)
        if w is not None:
            used[w] += n
    return verdicts


def test_caps_are_the_calls_limits(driver, tmp_path):
    assert run(driver, tmp_path, ["C"])[0] == [str(v) for v in (MANY_CAP, MANY_SUB_CAP, WIDE_CAP, WIDE_SUB_CAP)]
    assert MANY_SUB_CAP == 80 * 1024 - (43780 + 12 + 4096) and WIDE_SUB_CAP == 80 * 1024 - (35328 + 4096)


def test_the_fixed_packing_cases(driver, tmp_path):
    got = run(driver, tmp_path, ["P 40 40 40", "P 64 64", "P 64 1 64", "P 64 1 63", "P 1", "P 65", "P 0", "P 32 32 32 32 1"])
    assert got[0] == ["1", "1", "0"]             # 40 + 40 + 40: no word has room for the third
    assert got[1] == ["1", "1"]                  # 64 + 64: a word each
    assert got[2] == ["1", "1", "0"]             # 64 + 1 + 64: the 1 took the second word's first position
    assert got[3] == ["1", "1", "1"] and got[4] == ["1"] and got[5] == ["0"] and got[6] == ["0"]
    assert got[7] == ["1", "1", "1", "1", "0"]   # 128 bytes in all, and not one more


def test_group_fit_is_first_fit_over_every_prefix(driver, tmp_path):
    rng = np.random.default_rng(20261020)
    seqs = []
    for _ in range(600):
        hi = int(rng.choice([8, 24, 48, 64, 70]))
        seqs.append([int(x) for x in rng.integers(1, hi + 1, size=int(rng.integers(1, 14)))])
    got = run(driver, tmp_path, ["P " + " ".join(map(str, s)) for s in seqs])
    accepted = []
    seen = set()
    for s, g in zip(seqs, got):
        want = first_fit(s)
        assert [x == "1" for x in g] == want, s
        accepted.append([n for n, ok in zip(s, want) if ok])
        seen.update(want)
    assert seen == {True, False}
    # what the group took is what the library's pack_needles packs, and with one refused needle behind it, it does not
    lines = ["N " + " ".join(map(str, a)) for a in accepted if a]
    assert all(g == ["1"] for g in run(driver, tmp_path, lines))
    refused = [[n for n, ok in zip(s, first_fit(s)) if ok] + [s[first_fit(s).index(False)]] for s in seqs if False in first_fit(s)]
    refused = [r for s, r in zip([s for s in seqs if False in first_fit(s)], refused) if first_fit(s).index(False) == len(r) - 1]
    assert refused and all(g == ["0"] for g in run(driver, tmp_path, ["N " + " ".join(map(str, r)) for r in refused]))


def group_line(wide, queries):
    parts = ["G", str(int(wide)), str(len(queries))]
    for rx_bytes, needles in queries:
        parts += [str(rx_bytes), str(len(needles))] + [str(n) for n in needles]
    return " ".join(parts)


@pytest.mark.parametrize("wide,cap,sub_cap", [(False, MANY_CAP, MANY_SUB_CAP), (True, WIDE_CAP, WIDE_SUB_CAP)])
def test_the_reduced_regex_cap_applies_from_the_first_needle_on(driver, tmp_path, wide, cap, sub_cap):
    between = sub_cap + 4                        # table bytes the call holds without a needle table, not beside one
    assert sub_cap < between <= cap
    cases = [
        [(between, [])],                                         # no needle: the call's own cap
        [(cap, []), (4, [])],                                    # ... to the byte
        [(between, [8])],                                        # the query brings both: refused
        [(between, []), (0, [8])],                               # the needle arrives behind the tables: refused, the group stays
        [(0, [8]), (between, [])],                               # the tables arrive behind the needle: refused
        [(sub_cap, [8])],                                        # at the reduced cap: taken
        [(sub_cap - 8, [8]), (8, []), (4, []), (0, [8])],        # fills it, then one word too many; a needle still packs
        [(sub_cap - 2, [8])],                                    # the sum is padded to 4 before it is compared: still the cap
        [(sub_cap - 5, [8]), (2, []), (1, []), (3, [])],         # ... sub_cap - 3 and sub_cap - 2 pad to the cap, sub_cap + 1 pads past it
    ]
    got = run(driver, tmp_path, [group_line(wide, c) for c in cases])
    want = [[1], [1, 0], [0], [1, 0], [1, 0], [1], [1, 1, 0, 1], [1], [1, 1, 1, 0]]
    assert [[int(x) for x in g] for g in got] == want
    # random: needles by first-fit, bytes under the cap that holds at that point
    rng = np.random.default_rng(7 + wide)
    lines, wants = [], []
    for _ in range(300):
        used, n_needles, rx, qs, w = [0, 0], 0, 0, [], []
        for _ in range(int(rng.integers(1, 10))):
            needles = [int(x) for x in rng.integers(1, 50, size=int(rng.integers(0, 3)))]
            rx_bytes = int(rng.choice([0, 0, 1200, 9000, 20000, sub_cap - 1000]))
            trial, ok = list(used), True
            for n in needles:
                word = next((i for i in range(2) if trial[i] + n <= 64), None)
                ok = ok and word is not None
                if word is not None:
                    trial[word] += n
            limit = sub_cap if n_needles + len(needles) else cap
            ok = ok and ((rx + rx_bytes + 3) & ~3) <= limit
            if ok:
                used, n_needles, rx = trial, n_needles + len(needles), rx + rx_bytes
            qs.append((rx_bytes, needles))
            w.append(int(ok))
        lines.append(group_line(wide, qs))
        wants.append(w)
    assert [[int(x) for x in g] for g in run(driver, tmp_path, lines)] == wants
    assert any(0 in w for w in wants) and any(1 in w for w in wants)


def test_the_call_is_the_one_the_table_states(driver, tmp_path):
    table = {  # (regex, needles, wide, wide_rows) -> the call
        (0, 0, 0, 0): "bsg_match_rows_many", (1, 0, 0, 0): "bsg_match_rows_many_regex",
        (0, 1, 0, 0): "bsg_match_rows_many_substr", (1, 1, 0, 0): "bsg_match_rows_many_regex_substr",
        (0, 0, 1, 0): "bsg_match_rows_wide", (1, 0, 1, 0): "bsg_match_rows_wide",
        (0, 1, 1, 0): "bsg_match_rows_wide_substr", (1, 1, 1, 0): "bsg_match_rows_wide_substr",
        (0, 0, 1, 1): "bsg_match_rows_wide_rows", (1, 0, 1, 1): "bsg_match_rows_wide_rows",
        (0, 1, 1, 1): "bsg_match_rows_wide_substr_rows", (1, 1, 1, 1): "bsg_match_rows_wide_substr_rows",
        # the rows key alone is the wide route too (DeviceMatchWideRows implies the grouping of DeviceMatchWide)
        (0, 0, 0, 1): "bsg_match_rows_wide_rows", (1, 0, 0, 1): "bsg_match_rows_wide_rows",
        (0, 1, 0, 1): "bsg_match_rows_wide_substr_rows", (1, 1, 0, 1): "bsg_match_rows_wide_substr_rows",
    }
    keys = sorted(table)
    assert len(keys) == 16
    got = run(driver, tmp_path, ["K %d %d %d %d" % k for k in keys])
    assert [g[0] for g in got] == [table[k] for k in keys]
