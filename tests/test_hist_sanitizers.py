"""The bucket scanner's per-row lines under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/hist_scan_check.cpp, its own main, plain g++) runs minmax_scan_row plus hist_bucket_code — what k_bucket_rows inlines — over
every case of tests/hist_shapes.py and every truncation of it, the rows in heap blocks of exactly the words the kernel may read.
Decided rows give the restatement's slot, the rows the contract names give "U"; malformed and truncated rows need only a clean run.
Nothing is loaded into python."""
import os
import subprocess

import pytest

from tests import hist_restatement as HR
from tests import hist_shapes as HS
from tests import minmax_shapes as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scan_exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("hist_scan_asan")), "hist_scan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "hist_scan_check.cpp")], check=True, timeout=600)
    return path


def line(field, origin, width, n_buckets, row):
    return "%s %d %d %d %s\n" % (field.encode().hex(), origin, width, n_buckets, row.hex() if row else "-")


def test_the_bucket_scanner_on_the_cpu_under_the_sanitizers(scan_exe, tmp_path):
    cases = [(c.spec, c.row, c.undecided) for c in HS.CASES]
    cases += [(("ts", -40000, 1400, 60), HS.synth_row(i), False) for i in range(40)]
    malformed = [(("ts", 0, 1, 4), r) for r in MS.MALFORMED]
    path = tmp_path / "cases.txt"
    path.write_text("".join(line(*spec, row) for spec, row, _ in cases) + "".join(line(*spec, row) for spec, row in malformed))
    r = subprocess.run([scan_exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = r.stdout.split("\n")
    bad = [(cases[i], out[i]) for i in range(len(cases)) if out[i] != ("U" if cases[i][2] else str(HR.slot_of(cases[i][1], *cases[i][0])))]
    assert not bad, bad[:5]
    tail = out[len(cases) + len(malformed)]
    assert tail.startswith("done ") and int(tail.split()[1]) > 1000


def test_a_line_that_does_not_parse_is_reported(scan_exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("zz 0 1 4 7b7d\n" + line("ts", 0, 0, 4, b"{}") + line("ts", 0, 1, 1025, b"{}") + line("y" * 65, 0, 1, 4, b"{}") + line("ts", 0, 1, 4, b"{}"))
    r = subprocess.run([scan_exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:5] == ["?", "?", "?", "?", "6"]
