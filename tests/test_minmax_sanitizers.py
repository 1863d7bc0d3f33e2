"""host/minmax.hpp under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program (tests/minmax_check.cpp, its own main,
plain g++) folds every literal of the restatement, every shape and the malformed rows, and every one of those rows truncated at every
byte; its indexes equal the restatement's (the truncated rows need only a clean run).  A second program (tests/minmax_scan_check.cpp)
does the same with the DEVICE scanner's per-row function, which csrc/minmax.hip.h keeps as plain C++: the rows lie in heap blocks of
exactly the words the kernels may read, at every alignment, between bytes that must not be interpreted.  Nothing is loaded into python."""
import os
import subprocess

import pytest

from tests import minmax_restatement as MR
from tests import minmax_shapes as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "minmax_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("minmax_asan")), "minmax_check")
    # (-Wno-sign-compare: for the regex compiler's header, which range.hpp reaches through the expression trees)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc", "host"), "-o", path, SRC], check=True, timeout=600)
    return path


@pytest.fixture(scope="module")
def scan_exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("minmax_scan_asan")), "minmax_scan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "minmax_scan_check.cpp")], check=True, timeout=600)
    return path


def line(fields, row):
    return "%s %s\n" % (b"\0".join(f.encode() for f in fields).hex(), row.hex() if row else "-")


def want_line(fields, row):
    try:
        c = MR.row_contributions(row, fields)
    except ValueError:
        return "!"
    return " ".join("%d:%d:%d" % (i, c[f][0], c[f][1]) if f in c else "-" for i, f in enumerate(fields))


def test_every_literal_shape_and_truncation_under_the_sanitizers(exe, tmp_path):
    cases = [(["v"], ('{"w":[1,{"v":2}],"v":%s}' % lit).encode()) for lit in MR.LITERALS + [MR.BIG + "." + MR.BIG, "-0." + "0" * 40 + "1"]]
    cases += [(MS.FIELDS, s.row) for s in MS.SHAPES] + [(MS.FIELDS, r) for r in MS.MALFORMED]
    cases += [(MS.EIGHT, b'{"f0":1,"f7":-2.5,"f3":"x","f8":3}')]
    giants = [("1e99999999999999999999", "0:%d:%d" % (MR.I64_MAX, MR.I64_MAX)), ("-1e99999999999999999999", "0:%d:%d" % (MR.I64_MIN, MR.I64_MIN)),
              ("1e-99999999999999999999", "0:0:1"), ("-1e-99999999999999999999", "0:-1:0")]
    path = tmp_path / "cases.txt"
    path.write_text("".join(line(f, r) for f, r in cases) + "".join(line(["v"], ('{"v":%s}' % g).encode()) for g, _ in giants))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")
    got, tail = out[: len(cases) + len(giants)], out[len(cases) + len(giants)]
    bad = [(cases[i], got[i]) for i in range(len(cases)) if got[i] != want_line(*cases[i])]
    assert not bad, bad[:5]
    assert got[len(cases):] == [w for _, w in giants]
    done, truncated_ok, evals, passes = tail.split()
    assert done == "done" and int(evals) > 0 and int(passes) > 0
    # a proper prefix of a row that is one JSON object is never one (but for leading / trailing white space, which one shape has)
    assert int(truncated_ok) <= 4


def test_a_line_that_does_not_parse_and_bad_fields_are_reported(exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("zz 7b7d\n" + line(["a", "a"], b"{}") + line(["a" * 65], b"{}") + line(["a", ""], b"{}") + line(["a"], b"{}"))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "?" and all(o.startswith("?") and len(o) > 1 for o in out[1:4]) and out[4] == "-"


def test_the_device_scanner_on_the_cpu_under_the_sanitizers(scan_exe, tmp_path):
    """decided rows give the restatement's contribution, the rows the contract names give "U" (exponent on a field, backslash in a
    top-level key); malformed and truncated rows need only a clean run inside their own words"""
    lits = [(["v"], ('{"w":[1,{"v":2e5}],"v":%s,"x":3e5}' % lit).encode(), "e" in lit.lower()) for lit in MR.LITERALS + [MR.BIG + "." + MR.BIG, "-0." + "0" * 40 + "1"]]
    cases = lits + [(MS.FIELDS, s.row, s.undecided) for s in MS.SHAPES]
    cases += [(MS.EIGHT, b'{"f0":1,"f7":-2.5,"f3":"x","f8":3}', False), (MS.EIGHT, b'{"f0":1,"f7":-2.5e0}', True), (["ts"], MS.synth_row(3), False)]
    path = tmp_path / "cases.txt"
    path.write_text("".join(line(f, r) for f, r, _ in cases) + "".join(line(MS.FIELDS, r) for r in MS.MALFORMED))
    r = subprocess.run([scan_exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = r.stdout.split("\n")
    bad = [(cases[i], out[i]) for i in range(len(cases)) if out[i] != ("U" if cases[i][2] else want_line(cases[i][0], cases[i][1]))]
    assert not bad, bad[:5]
    assert out[len(cases) + len(MS.MALFORMED)].startswith("done ")
