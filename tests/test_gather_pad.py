"""bsh::gather_lds_pad (bloomsearch_amd/csrc/host/probe_plan.hpp) on the host, no GPU: tests/gather_pad_check.cpp, a stand-alone program
built with g++ (with -fsanitize=address,undefined where the toolchain has the runtimes).  The gather kernels hold no LDS, so the dynamic
LDS a launch asks for is what caps their workgroups per CU.  Asserted over 0 .. 8 workgroups per CU: 0 and everything above 4 (what the
kernels' 8 waves a workgroup allow anyway) give no pad; 1 .. 4 give a pad of which exactly that many fit into a CU's 160 KiB — also after
the hardware has rounded the request up to its allocation unit —, no larger than the attribute bsg_open sets for the kernels; the planner's
own rule is one of these values."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU_LDS = 160 * 1024
N = 8


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather_pad")
    exe = d / "gather_pad_check"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
            os.path.join(ROOT, "tests", "gather_pad_check.cpp")]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if san.returncode != 0:                                   # (a toolchain without the sanitizer runtimes: the plain program)
        subprocess.run(base, check=True, timeout=300)
    r = subprocess.run([str(exe), str(d / "answers.bin"), str(N)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    w = [int(x) for x in np.fromfile(d / "answers.bin", dtype="<u8")]
    assert len(w) == N + 1 + 6
    return w[: N + 1], dict(zip(("cu_lds", "unit", "opt_in", "pad_max", "max_wgs", "rule"), w[N + 1:]))


def test_the_constants_are_the_cu_s(answers):
    _, c = answers
    assert c["cu_lds"] == CU_LDS and c["opt_in"] == 64 * 1024 and c["max_wgs"] == 4
    assert c["opt_in"] < c["pad_max"] <= CU_LDS and c["unit"] > 0 and CU_LDS % c["unit"] == 0
    assert 0 <= c["rule"] <= 8


def test_zero_and_more_than_four_workgroups_mean_no_pad(answers):
    pad, _ = answers
    assert pad[0] == 0
    assert all(pad[n] == 0 for n in range(5, N + 1))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_exactly_the_requested_workgroups_fit(answers, n):
    pad, c = answers
    assert pad[n] > 0 and CU_LDS // pad[n] == n
    granted = (pad[n] + c["unit"] - 1) // c["unit"] * c["unit"]           # what the hardware allocates for the request
    assert CU_LDS // granted == n
    assert pad[n] <= c["pad_max"]                                          # within the kernels' opt-in attribute (gather_lds_pad(1))
    assert pad[1] == max(pad)
