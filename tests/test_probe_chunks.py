"""bsh::pipeline_chunks (bloomsearch_amd/csrc/host/probe_plan.hpp) on the host, no GPU: tests/probe_chunks_check.cpp, a stand-alone
program built with g++ (with -fsanitize=address,undefined where the toolchain has the runtimes) and run over every group of up to
300 arenas under every kind of key 27 value.  Asserted: the chunk sizes are positive, sum to the group and are the same on a second
call; ONE chunk under every excluding condition (key 1, a launch that does not gather, a batch that is not a few-term identity
batch, more than one group, fold / fuse / tail split selected, a group of one arena) whatever the key; with key 0 one chunk below
either threshold and the default count above both; with key n exactly min(n, arenas) chunks that differ by at most one arena,
or, with a last-chunk percent, a last chunk no larger than the others."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 300
KEYS = [0, 1, 2, 3, 4, 6, 9, 300, 301, 0xFFFF, 3 | (50 << 16), 4 | (25 << 16), 2 | (100 << 16), 6 | (1 << 16), 3 | (0xFF << 16), 3 | (2 << 24), (1 << 24), 4 | (50 << 16) | (1 << 24)]
OK = (1, 1, 1, 0)                                             # gathers, identity_few, n_groups, other_route
EXCLUDED = [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 2, 0), (1, 1, 5, 0), (1, 1, 1, 1), (0, 0, 3, 1)]
BIG = 1 << 40                                                 # blocks: above any threshold


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("probe_chunks") / "probe_chunks_check"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
            os.path.join(ROOT, "tests", "probe_chunks_check.cpp")]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if san.returncode != 0:                                   # (a toolchain without the sanitizer runtimes: the plain program)
        subprocess.run(base, check=True, timeout=300)
    return exe


def run_driver(exe, tmp_path, cases):
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8"), np.asarray(cases, dtype="<u8").ravel()])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    w = [int(x) for x in np.fromfile(tmp_path / "answers.bin", dtype="<u8")]
    out, at = [], 0
    for _ in cases:
        out.append(w[at + 1: at + 1 + w[at]])
        at += 1 + w[at]
    assert len(w) == at + 4
    return out, dict(zip(("min_arenas", "min_blocks", "chunks", "last_pct"), w[at:]))


def test_sizes_are_positive_sum_to_the_group_and_have_the_asked_count(driver, tmp_path):
    cases = [(n, BIG) + OK + (key,) for n in range(0, N_MAX + 1) for key in KEYS]
    got, dflt = run_driver(driver, tmp_path, cases)
    assert 2 <= dflt["chunks"] <= 16 and 1 <= dflt["last_pct"] <= 100 and dflt["min_arenas"] > 20      # (a 20-arena run keeps two dispatches)
    for (n, _, _, _, _, _, key), sizes in zip(cases, got):
        assert all(s > 0 for s in sizes) and sum(sizes) == n, (n, key, sizes)
        want_n, pct = key & 0xFFFF, min((key >> 16) & 0xFF, 100) or 100
        if n < 2 or key == 1:
            assert len(sizes) == min(n, 1), (n, key, sizes)
            continue
        if want_n < 2:                                        # the planner decides
            if n < dflt["min_arenas"]:
                assert sizes == [n], (n, key, sizes)
                continue
            want_n, pct = dflt["chunks"], dflt["last_pct"]
        assert len(sizes) == min(want_n, n), (n, key, sizes)
        if pct == 100:
            assert max(sizes) - min(sizes) <= 1, (n, key, sizes)
        else:
            assert sizes[-1] <= min(sizes[:-1]) and max(sizes[:-1]) - min(sizes[:-1]) <= 1, (n, key, sizes)
            assert sizes[-1] == max(1, n * pct // (100 * len(sizes))), (n, key, sizes)


def test_one_chunk_under_every_excluding_condition(driver, tmp_path):
    cases = [(n, BIG) + ex + (key,) for n in range(0, N_MAX + 1) for key in KEYS for ex in EXCLUDED]
    cases += [(n, BIG) + OK + (1,) for n in range(0, N_MAX + 1)]
    got, _ = run_driver(driver, tmp_path, cases)
    for c, sizes in zip(cases, got):
        assert sizes == ([c[0]] if c[0] else []), (c, sizes)


def test_the_planner_needs_both_thresholds(driver, tmp_path):
    _, dflt = run_driver(driver, tmp_path, [(2, 2) + OK + (0,)])
    a, b = dflt["min_arenas"], dflt["min_blocks"]
    cases = [(n, blocks) + OK + (0,) for n in (2, a - 1, a, a + 1, N_MAX) for blocks in (0, b - 1, b, b + 1, BIG)]
    got, _ = run_driver(driver, tmp_path, cases)
    for (n, blocks, *_), sizes in zip(cases, got):
        assert (len(sizes) > 1) == (n >= a and blocks >= b), (n, blocks, sizes)
        assert sum(sizes) == n and all(s > 0 for s in sizes)
    # a forced count ignores both
    forced, _ = run_driver(driver, tmp_path, [(2, 0) + OK + (2,), (a - 1, 1) + OK + (3,)])
    assert [len(s) for s in forced] == [2, 3]
