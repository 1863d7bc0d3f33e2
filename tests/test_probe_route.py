"""Gather or stream, decided on the host (no GPU): tests/probe_route_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/probe_plan.hpp, compared with the rule restated here in Python's unbounded integers: a few-term launch
gathers when EVERY referenced kind has terms x k x cost x blocks < sum_words x 8 (strictly), never for a many-term batch, a launch
without kinds or without blocks, and — unless the cost is 0 — never when a kind holds filters beyond the LDS budget.  The program is built under AddressSanitizer and UBSan as a plain host program."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("probe_route") / "probe_route_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "probe_route_check.cpp")], check=True, timeout=300)
    return exe


def want(kinds, n_blocks, many, cost):
    """kinds: (sum_words, terms, k) or (sum_words, terms, k, unstaged_words)"""
    if many or not kinds or n_blocks == 0:
        return 0
    if cost != 0 and any(len(kd) > 3 and kd[3] for kd in kinds):
        return 0
    return int(all(kd[1] * kd[2] * cost * n_blocks < kd[0] * 8 for kd in kinds))


def ask(exe, tmp_path, cases):
    words = [len(cases)]
    for kinds, n_blocks, many, cost in cases:
        words += [len(kinds), n_blocks, int(many), cost] + [x for kd in kinds for x in (kd[0], kd[3] if len(kd) > 3 else 0, kd[1], kd[2])]
    np.asarray(words, dtype="<u8").tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = [int(x) for x in np.fromfile(tmp_path / "answers.bin", dtype="<u8")]
    assert len(got) == 2 * len(cases)
    ask.bytes = got[1::2]
    return got[0::2]


def test_the_named_cases(driver, tmp_path):
    c2 = (4395 * 1000 * 20, 29, 10)                     # the headline's group: 20 arenas x 1 000 FieldToken filters of 35 160 bytes
    cases = [
        ([c2], 0, False, 64),                           # zero blocks
        ([(0, 29, 10)], 1000, False, 0),                # one kind, every filter nil: nothing to gather, even at cost 0
        ([c2, (0, 5, 10)], 20000, False, 0),            # ... beside a kind that would gather
        ([(125, 10, 10)], 1, False, 10),                # equality at the threshold: 10 * 10 * 10 * 1 == 125 * 8 streams
        ([(125, 10, 10)], 1, False, 9),                 # ... one below gathers
        ([(126, 10, 10)], 1, False, 10),
        ([c2], 20000, True, 0),                         # a many-term batch is refused whatever the cost
        ([c2], 20000, False, 0),                        # cost 0: gather
        ([c2], 20000, False, U32),                      # cost 2^32 - 1: stream
        ([c2], 20000, False, 64), ([c2], 20000, False, 121), ([c2], 20000, False, 122), ([c2], 20000, False, 256),
        ([(4395 * 20000, 77, 10)], 20000, False, 64),   # the C4 batch's 77 terms at the sector size: streams
        ([], 1000, False, 0),                           # no referenced kind
        # filters beyond the LDS budget (64 blocks x 1.04 MB): the streaming kernels gather them per block already; only cost 0 moves the launch
        ([(64 * 130000, 29, 10, 64 * 130000)], 64, False, 96), ([(64 * 130000, 29, 10, 64 * 130000)], 64, False, 0), ([(64 * 130000, 29, 10, 0)], 64, False, 96),
        ([c2, (1 << 20, 3, 10, 1 << 19)], 20000, False, 1), ([c2, (1 << 20, 3, 10, 1 << 19)], 20000, False, 0),
        # products near and beyond 2^64 (and, for arguments no launch has, beyond 2^128): no wrap-around decides
        ([(U64 // 8, U32, U32)], 1, False, 1), ([(U64 // 8, U32, U32)], 2, False, 1), ([(U64, U32, U32)], U64, False, U32),
        ([(U64, U32, U32)], U64, False, 0), ([(U64, 1, 1)], U64, False, 7), ([(U64, 1, 1)], U64, False, 8), ([(U64, 1, 1)], U64, False, 9),
        ([(1 << 61, 1 << 16, 1 << 16)], 1 << 32, False, 1), ([((1 << 61) + 1, 1 << 16, 1 << 16)], 1 << 32, False, 1),
        ([(1, U32, U32)], U64, False, U32),
    ]
    got = ask(driver, tmp_path, cases)
    assert got == [want(*c) for c in cases]
    # ... and what the restated rule says of the cases the contract names
    assert got[:9] == [0, 0, 0, 0, 1, 1, 0, 1, 0] and got[15:20] == [0, 1, 1, 0, 1]
    assert want([(125, 10, 10)], 1, False, 10) == 0 and want([c2], 20000, False, 121) == 1 and want([c2], 20000, False, 122) == 0


def test_random_launches_agree_with_unbounded_integers(driver, tmp_path):
    rng = np.random.default_rng(31)
    cases = []
    for _ in range(4000):
        kinds = []
        for _ in range(int(rng.integers(0, 4))):
            terms, k = int(rng.integers(0, 200)), int(rng.integers(0, 31))
            blocks = int(rng.integers(0, 5000))
            cost = int(rng.choice([0, 1, 8, 64, 128, 256, 1 << 20, U32]))
            base = terms * k * cost * blocks // 8                                  # sums straddling the threshold, and anything else
            sw = max(0, base + int(rng.integers(-2, 3))) if rng.random() < 0.6 else int(rng.integers(0, 1 << 40))
            kinds.append((sw, terms, k, int(rng.integers(0, sw + 1)) if rng.random() < 0.15 else 0))
        cases.append((kinds, blocks if kinds else 7, rng.random() < 0.1, cost if kinds else 64))
    got = ask(driver, tmp_path, cases)
    assert got == [want(*c) for c in cases]
    assert 0.05 < sum(got) / len(got) < 0.95


def test_the_binding_states_the_librarys_default_cost():
    import re
    from bloomsearch_amd import _lib
    src = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "bloomgpu.hip")).read()
    found = re.findall(r"uint32_t gather_cost = (\d+);", src)
    assert len(found) == 1 and int(found[0]) == _lib.GATHER_COST_DEFAULT


def test_bytes_reported_for_a_gathered_launch(driver, tmp_path):
    """bsg_timing.stream_bytes of a gathered launch: the 128-byte lines terms x k bit tests are expected to touch, L (1 - exp(-t / L)) per
    filter of L lines — never more than the filters hold, nothing for nil filters or a launch without blocks."""
    import math
    c2 = (4395 * 1000 * 20, 29, 10)
    cases = [([c2], 20000, False, 0), ([c2], 0, False, 0), ([(0, 29, 10)], 1000, False, 0), ([(16, 128, 20)], 1, False, 0),
             ([c2, (16 * 20000, 3, 1)], 20000, False, 0), ([(U64 // 8, U32, U32)], 1, False, 0)]
    ask(driver, tmp_path, cases)
    got = ask.bytes

    def model(sum_words, terms, k, n_blocks):
        if not n_blocks or not sum_words:
            return 0
        lines = sum_words * 8 / 128 / n_blocks
        return min(lines * (1 - math.exp(-terms * k / lines)) * 128 * n_blocks, sum_words * 8)

    assert abs(got[0] - model(*c2, 20000)) <= 1 + 1e-9 * got[0]                          # (the library truncates to whole bytes)
    assert 178 * 128 * 20000 < got[0] < 180 * 128 * 20000                                # C2: 179 of a block's 275 lines
    assert got[1] == 0 and got[2] == 0
    assert 0.99 * 128 <= got[3] <= 128                                                   # a one-line filter tested 2 560 times: its line
    assert abs(got[4] - model(*c2, 20000) - model(16 * 20000, 3, 1, 20000)) <= 2 + 1e-9 * got[4]
    assert got[5] <= U64 // 8 * 8
