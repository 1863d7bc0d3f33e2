"""host/range.hpp under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program (tests/range_check.cpp, its own main,
plain g++) runs every literal of the restatement against every pair of bounds — the 40-digit integers, the int64 edges and the
exponent forms among them — and its verdicts equal the restatement's.  Nothing is loaded into python."""
import os
import subprocess

import pytest

from tests import range_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "range_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("range_asan")), "range_check")
    # (-Wno-sign-compare: for the regex compiler's header, which range.hpp reaches through the expression trees)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc", "host"), "-o", path, SRC], check=True, timeout=600)
    return path


def spec(b):
    return "-" if b is None else ("o" if b[1] else "c") + str(b[0])


def test_every_literal_and_bound_under_the_sanitizers(exe, tmp_path):
    cases = [(lit, lo, hi) for lit in RR.LITERALS for lo, hi in RR.BOUND_PAIRS]
    cases += [(RR.BIG + "." + RR.BIG, lo, hi) for lo, hi in RR.BOUND_PAIRS] + [("-0." + "0" * 40 + "1", lo, hi) for lo, hi in RR.BOUND_PAIRS]
    # exponents no Fraction could hold: the verdicts are stated (far above int64 max; just above 0; -1.23...)
    giants = [("1e99999999999999999999", None, (RR.I64_MAX, False), "0"), ("1e-99999999999999999999", (0, True), (1, False), "1"),
              ("-1e99999999999999999999", (RR.I64_MIN, False), None, "0"), ("-" + RR.BIG + "e-39", (-2, False), (-1, True), "1")]
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %s %s\n" % (lit, spec(lo), spec(hi)) for lit, lo, hi in cases + [g[:3] for g in giants]))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    verdicts, tail = r.stdout.split("\n")[:2]
    want = "".join("1" if RR.inside(RR.exact(lit), lo, hi) else "0" for lit, lo, hi in cases)
    assert verdicts[len(want):] == "".join(g[3] for g in giants)
    verdicts = verdicts[:len(want)]
    bad = [cases[i] for i in range(len(want)) if verdicts[i] != want[i]]
    assert not bad, bad[:5]
    assert tail.split()[1:] == ["64", "64"]


def test_a_line_that_does_not_parse_is_reported(exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("5 c1\n5 x1 -\n5 c9223372036854775808 -\n5 c-9223372036854775808 c9223372036854775807\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "???1", (r.stdout, r.stderr[-2000:])
