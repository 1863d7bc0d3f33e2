"""The chunk plan of the row upload on the host (no GPU): tests/row_chunks_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/row_chunks.hpp — the code RowUpload (bloomgpu.hip) cuts and copies the rows of bsg_ingest_rows and
bsg_match_rows by.  Reference: the two loops that header replaced, restated below from ingest_rows_part (ingest_api.inc; the walk is
RowWalk's there now) and match_rows_on (match_api.inc) as they stood when each path still planned its own chunks.  On top of the comparison, what the
kernels rely on is asserted by itself: chunks are whole 256-row workgroups, the byte ranges of successive copies are disjoint (no
copy rewrites a byte a running kernel may read) and each reaches through the aligned 8-byte word that holds its last row's last
byte (the walker reads whole words)."""
import os
import subprocess
from bisect import bisect_right

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_CHUNK = [1 << 16, 1 << 20, 64 << 20]
N_ROWS = [1, 255, 256, 257, 3000]


def ingest_plan_before(row_off, n_rows, first):
    """ingest_rows_part: cuts on the caller's offsets, byte ranges in the same coordinates"""
    n_bytes = row_off[n_rows]
    cuts, chunk_bytes, r = [0], first, 0
    while r < n_rows:
        lim = row_off[r] + chunk_bytes
        if chunk_bytes < 4 * first:
            chunk_bytes *= 2
        e = bisect_right(row_off, lim, r + 1, n_rows + 1) - 1
        e = max(e, r + 1)
        if e < n_rows:
            e = min(n_rows, (e + 255) // 256 * 256)
        cuts.append(e)
        r = e
    ranges, copied_to = [], 0
    for c in range(len(cuts) - 1):
        b0 = (row_off[cuts[c]] & ~7) if c == 0 else copied_to
        b1 = max(b0, min(n_bytes, (row_off[cuts[c + 1]] + 23) & ~7))
        copied_to = b1
        ranges.append((b0, b1))
    return cuts, ranges


def match_plan_before(row_off, r0, r1, first):
    """match_rows_on: rows [r0, r1) rebased to the run's first byte, cuts and byte ranges on the rebased offsets"""
    n_rows, byte0 = r1 - r0, row_off[r0]
    n_bytes = row_off[r1] - byte0
    local_off = [row_off[r0 + r] - byte0 for r in range(n_rows + 1)]
    cuts, chunk_bytes, r = [0], first, 0
    while r < n_rows:
        lim = local_off[r] + chunk_bytes
        if chunk_bytes < 4 * first:
            chunk_bytes *= 2
        c1 = bisect_right(local_off, lim, r + 1, len(local_off)) - 1
        c1 = max(c1, r + 1)
        if c1 < n_rows:
            c1 = min(n_rows, (c1 + 255) // 256 * 256)
        cuts.append(c1)
        r = c1
    ranges, copied_to = [], 0
    for c in range(len(cuts) - 1):
        b0 = (local_off[cuts[c]] & ~7) if c == 0 else copied_to
        b1 = max(b0, min(n_bytes, (local_off[cuts[c + 1]] + 23) & ~7))
        copied_to = b1
        ranges.append((b0, b1))
    return local_off, cuts, ranges


def offset_tables():
    """(name, first_chunk_bytes, offsets): every shape for every n_rows and first-chunk size, seeded"""
    out = []
    for first in FIRST_CHUNK:
        for n in N_ROWS:
            for shape in ("small", "chunky", "empties", "giant", "shifted"):
                rng = np.random.default_rng([first, n, len(shape)])
                if shape == "small":                       # log lines: the whole table is one chunk or a few
                    lens = rng.integers(1, 400, n)
                elif shape == "chunky":                    # ~40 rows per first chunk: many chunks, the doubling and the 4x cap
                    lens = rng.integers(1, first // 20, n)
                elif shape == "empties":                   # runs of empty rows, also first and last
                    lens = rng.integers(0, first // 10, n) * (rng.random(n) < 0.5)
                    lens[0] = lens[-1] = 0
                elif shape == "giant":                     # one row larger than four chunks among small ones
                    lens = rng.integers(0, first // 50 + 2, n)
                    lens[n // 2] = 20 * first + 5
                else:                                      # the first offset is neither 0 nor a multiple of 8
                    lens = rng.integers(1, first // 30, n)
                start = 8 * int(rng.integers(1, 1000)) + 3 if shape == "shifted" else 0
                off = [start] + (start + np.cumsum(lens.astype(np.uint64))).astype(np.uint64).tolist()
                out.append((f"{shape}-n{n}-first{first}", first, [int(x) for x in off]))
    return out


def run_driver(tmp_path, cases):
    exe = tmp_path / "row_chunks_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "row_chunks_check.cpp")], check=True, timeout=120)
    words = [len(cases)]
    for first, off in cases:
        words += [first, len(off) - 1] + off
    inp = tmp_path / "cases.bin"
    np.asarray(words, dtype="<u8").tofile(inp)
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == 2 * len(cases) + 1 and lines[-1] == ""
    got = []
    for i in range(len(cases)):
        cuts = [int(x) for x in lines[2 * i].split()]
        flat = [int(x) for x in lines[2 * i + 1].split()]
        got.append((cuts, list(zip(flat[0::2], flat[1::2]))))
    return got


def check_plan(name, off, cuts, ranges):
    n_rows, n_bytes = len(off) - 1, off[-1]
    assert cuts[0] == 0 and cuts[-1] == n_rows, name
    assert all(a < b for a, b in zip(cuts, cuts[1:])), name
    assert all(c % 256 == 0 for c in cuts[:-1]), name
    assert len(ranges) == len(cuts) - 1, name
    assert ranges[0][0] <= off[0] and ranges[0][0] % 8 == 0, name
    for c, (b0, b1) in enumerate(ranges):
        assert b0 <= b1 <= n_bytes, (name, c)
        if c:
            assert b0 == ranges[c - 1][1], (name, c)          # disjoint and ascending, nothing left out between them
        end = off[cuts[c + 1]]                                # one past the last byte of the chunk's last row
        assert b1 >= min(n_bytes, (end + 7) & ~7), (name, c)


def test_the_header_plans_what_both_paths_planned_and_keeps_the_copy_ranges_disjoint(tmp_path):
    tables = offset_tables()
    assert len(tables) == len(FIRST_CHUNK) * len(N_ROWS) * 5
    cases, want = [], []
    for name, first, off in tables:
        n = len(off) - 1
        cases.append((first, off))                            # as bsg_ingest_rows hands its offsets over
        want.append((name + "/ingest", off) + ingest_plan_before(off, n, first))
        local_off, cuts, ranges = match_plan_before(off, 0, n, first)
        cases.append((first, local_off))                      # as bsg_match_rows does: rebased to the run's first byte
        want.append((name + "/match", local_off, cuts, ranges))
        if n >= 257:                                          # a run in the middle of the table (one device's part of a call)
            r0, r1 = 64, n - 1
            local_off, cuts, ranges = match_plan_before(off, r0, r1, first)
            cases.append((first, local_off))
            want.append((name + "/match-run", local_off, cuts, ranges))
    got = run_driver(tmp_path, cases)
    n_multi = 0
    for (name, off, cuts, ranges), (got_cuts, got_ranges) in zip(want, got):
        assert got_cuts == cuts, name
        assert got_ranges == ranges, name
        check_plan(name, off, got_cuts, got_ranges)
        n_multi += len(got_cuts) > 3
    assert n_multi >= len(tables) // 3                        # the tables do exercise the doubling, not only one-chunk plans


@pytest.mark.parametrize("first", FIRST_CHUNK)
def test_no_rows_is_a_plan_of_no_chunks(tmp_path, first):
    (cuts, ranges), = run_driver(tmp_path, [(first, [40])])
    assert cuts == [0] and ranges == []
