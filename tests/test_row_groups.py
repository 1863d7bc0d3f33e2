"""The order a streaming ingest walks the rows of an upload chunk in (no GPU): tests/row_groups_check.cpp, built with plain g++
under AddressSanitizer and UBSan against bloomsearch_amd/csrc/host/row_groups.hpp — the code bsg_ingest_append_rows groups every
chunk by before k_ingest_rows_sets walks it.  Reference: Python's stable sort of the chunk's row indices by set.  What the kernel
relies on is asserted by itself: the chunk's positions hold a permutation of the chunk's own rows (a row is walked exactly once,
and only rows whose bytes have landed), the sets ascend (a wave stays inside one set or two), rows of one set keep their arrival
order, and nothing outside the chunk's range of either array is written (the chunk before may still be read by its kernel)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    out = []
    rng = np.random.default_rng(5)
    for n_sets, n_rows in [(1, 1), (1, 70), (3, 200), (4, 300), (16, 1000), (40, 180), (1000, 64), (5000, 3), (7, 0), (2, 257)]:
        for shape in ("interleaved", "random", "one_set", "descending"):
            if shape == "interleaved":
                s = np.arange(n_rows) % n_sets
            elif shape == "random":
                s = rng.integers(0, n_sets, n_rows)
            elif shape == "one_set":
                s = np.full(n_rows, n_sets - 1)
            else:
                s = (n_sets - 1) - np.arange(n_rows) % n_sets
            for r0, r1 in {(0, n_rows), (n_rows // 3, n_rows), (n_rows // 4, n_rows // 2), (n_rows, n_rows)}:
                out.append((n_sets, n_rows, r0, r1, s.astype(np.uint32)))
    return out


def run_driver(tmp_path, cs):
    exe = tmp_path / "row_groups_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "row_groups_check.cpp")],
                   check=True, timeout=120)
    words = [np.asarray([len(cs)], dtype="<u4")]
    for n_sets, n_rows, r0, r1, s in cs:
        words += [np.asarray([n_sets, n_rows, r0, r1], dtype="<u4"), s.astype("<u4")]
    inp = tmp_path / "cases.bin"
    np.concatenate(words).tofile(inp)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def test_chunks_are_stably_grouped_by_set_and_nothing_else_is_written(tmp_path):
    cs = cases()
    bad = (3, 10, 0, 10, np.array([0, 1, 2, 0, 3, 1, 7, 0, 0, 0], dtype=np.uint32))     # row 4 names set 3 of 3
    lines = run_driver(tmp_path, cs + [bad])
    at = 0
    for n_sets, n_rows, r0, r1, s in cs:
        what = (n_sets, n_rows, r0, r1)
        assert int(lines[at]) == n_rows, what
        order = [int(x) for x in lines[at + 1].split()]
        sets = [int(x) for x in lines[at + 2].split()]
        assert lines[at + 3] == "1", what
        at += 4
        assert sorted(order) == list(range(r0, r1)), what                                    # a permutation of the chunk's own rows
        assert order == sorted(range(r0, r1), key=lambda r: int(s[r])), what                 # Python's sort is stable: sets ascend, arrival order kept
        assert sets == [int(s[r]) for r in order], what
    assert int(lines[at]) == 4 and lines[at + 1:] == [""]
