"""The program evaluator's row-span body (eval_role_rows: a workgroup evaluates a span of 64-block groups of one arena for a chunk
of 256 queries and writes the survivor words out of an LDS stage in 16-byte slots) against the CPU oracle's probe_batch, and the
body it replaces (BSG_LAB_EVAL_ROWS=0) against the same arrays.

The lab variables are read once per process, so every mode is a worker process of its own (tests/_eval_rows_worker.py), started
once per session; the cases below only read what their worker reported.  Modes:
  old       BSG_LAB_EVAL_ROWS=0 BSG_LAB_EVAL_TILE=4   the tiled body at every shape
  rows      BSG_LAB_EVAL_TILE=4                        the row spans at every shape (small launches would keep one group per workgroup)
  default   nothing set                                what the host chooses by itself
Shapes: arenas of G = 1, 2, 8, 9, 16, 17, 18 and 33 groups (tail mask, a span's edge, a partial second span, G odd and no multiple of
the span), 1 .. 600 queries (a chunk's edge, rows beyond n_queries, the last partial 16-byte slot), programs from nil to deeper than
either body's LDS, one and two verdict words, groups of arenas with different G / out_off / v_off through the kernel-argument and
the device-memory table, the streamed, gathered and chunked routes (the evaluation inside k_gather_fused)."""
import json
import os
import subprocess
import sys

import pytest

from tests import _eval_rows_worker as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = {"old": {"BSG_LAB_EVAL_ROWS": "0", "BSG_LAB_EVAL_TILE": "4"}, "rows": {"BSG_LAB_EVAL_TILE": "4"}, "default": {}}


@pytest.fixture(scope="session")
def reports(tmp_path_factory):
    """{mode: {case: "ok" | what differs}}: one worker per mode, one after the other, the oracle's arrays shared through a directory"""
    root = os.path.join(HERE, "..")
    base = tmp_path_factory.mktemp("eval_rows")
    want_dir = base / "want"
    want_dir.mkdir()
    out = {}
    for mode, extra in MODES.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("BSG_LAB_EVAL_")}
        env.update(extra, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        path = base / (mode + ".json")
        r = subprocess.run([sys.executable, os.path.join(HERE, "_eval_rows_worker.py"), str(path), str(want_dir)], env=env, cwd=root,
                           capture_output=True, text=True, timeout=600)
        out[mode] = (json.load(open(path)) if path.exists() else {}, r.returncode, r.stdout[-2000:] + r.stderr[-2000:])
        if r.returncode != 0:
            break                                             # a worker that died: nothing more runs on the device in this fixture
    return out


@pytest.mark.parametrize("case", W.case_names())
@pytest.mark.parametrize("mode", list(MODES))
def test_survivors_equal_the_oracle(reports, mode, case):
    assert mode in reports, "the worker of mode %r did not run: one before it died" % mode
    results, rc, tail = reports[mode]
    assert case in results, "the worker of mode %r ended (exit status %d) before this case: %s" % (mode, rc, tail)
    assert results[case] == "ok", results[case]


@pytest.mark.parametrize("mode", list(MODES))
def test_the_worker_ran_every_case(reports, mode):
    assert mode in reports
    results, rc, tail = reports[mode]
    assert rc == 0 and sorted(results) == sorted(W.case_names()), tail
