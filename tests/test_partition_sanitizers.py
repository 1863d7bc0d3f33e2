"""The keyed ingest's per-row functions under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/partition_scan_check.cpp, its own main, plain g++) runs the DEVICE scanner — csrc/partition.hip.h keeps it as plain C++ — and
the host's partition_key (host/partition.hpp, the body of bsh_partition_key) over every shape, at every alignment, in heap blocks of
exactly the words the kernels may read, and over every truncation of every shape.  Nothing is loaded into python."""
import os
import subprocess

import pytest

from tests import partition_restatement as PR
from tests import partition_shapes as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("partition_asan")), "partition_scan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc", "host"), "-o", path, os.path.join(ROOT, "tests", "partition_scan_check.cpp")],
                   check=True, timeout=600)
    return path


def line(name, row):
    return "%s %s\n" % (name.encode().hex(), row.hex() if row else "-")


def hexed(b):
    return b.hex() if b else "-"


MALFORMED = [b"", b"{", b'{"p"', b'{"p":', b'{"p":"open', b'{"p":tr', b'{"p":-', b'{"p":"x\\', b"[1,2]", b'"p"', b'{"p":1}}}}', b"}}}{", b'{"a":"\\']


def test_every_shape_alignment_and_truncation_under_the_sanitizers(exe, tmp_path):
    cases = [(s.field, s.row) for s in PS.SHAPES]
    path = tmp_path / "cases.txt"
    path.write_text("".join(line(f, r) for f, r in cases) + "".join(line("p", r) for r in MALFORMED))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = r.stdout.split("\n")
    for s, got in zip(PS.SHAPES, out):
        dev, hst = got.split(" ")
        assert hst == "H:" + hexed(s.text), (s.name, got)
        assert dev == ("U" if s.undecided else "D:" + hexed(s.text)), (s.name, got)
        assert s.undecided == (not PR.device_decides(s.row, s.field))
    tail = out[len(cases) + len(MALFORMED)]
    assert tail.startswith("done ") and int(tail.split()[1]) == sum(len(r) for _, r in cases) + sum(len(r) for r in MALFORMED)
    # the host refuses every malformed row; the device scanner's answer for them is unspecified, its run clean
    assert all(o.endswith(" !") for o in out[len(cases): len(cases) + len(MALFORMED)])


def test_a_line_that_does_not_parse_is_reported(exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("zz 7b7d\n" + "- 7b7d\n" + line("n" * 65, b"{}") + line("p", b"{}"))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:4] == ["?", "?", "?", "D:- H:-"]
