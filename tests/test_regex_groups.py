"""The arithmetic of FieldRegex conditions in a batch on the host (no GPU): tests/regex_groups_check.cpp, built with plain g++
against bloomsearch_amd/csrc/host/regex_groups.hpp — the code bsg_match_rows_many_regex (match_api.inc) builds its table blob and
user masks by and the engine mirror (engine.hpp match_rows_device_many) closes its groups by.  References: co_active_bound against
a brute-force count over every path that a set of random dotted fields can cover; the table-byte estimate against its stated
formula (16 header bytes, 8 user-mask bytes in the batched blob, 256 + 2 * states * classes padded to 4, the field) and against
the blob build_blob emits for the patterns of tests/test_match_regex_gpu.py::PY; user masks against the programs of
query.CompiledRowQueryBatch."""
import os
import re
import subprocess

import numpy as np
import pytest

from bloomsearch_amd import _lib, query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_CAP, MANY_CAP = 44544, 38140          # bloomgpu.h: bsg_match_rows_regex, bsg_match_rows_many_regex
OK, TOO_MANY, PATTERN, OVER_CAP = 0, 1, 2, 3


def py_patterns():
    """the keys of tests/test_match_regex_gpu.py::PY, read from its source (importing it needs the GPU suite's helpers)"""
    src = open(os.path.join(ROOT, "tests", "test_match_regex_gpu.py"), encoding="utf-8").read()
    body = src[src.index("PY = {"): src.index("PATTERNS = sorted(PY)")]
    ns = {}
    exec(body, ns)
    return sorted(ns["PY"])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("regex_groups") / "regex_groups_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-sign-compare",     # (regex_dfa.hpp compares digits as the library's build does)
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "regex_groups_check.cpp")], check=True, timeout=600)
    return exe


def hx(s):
    b = s if isinstance(s, bytes) else s.encode("utf-8")
    return b.hex() if b else "-"


def run(exe, tmp_path, lines):
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt"), str(tmp_path / "answers.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [[int(x) for x in l.split()] for l in (tmp_path / "answers.txt").read_text().splitlines()]
    assert len(out) == len(lines)
    return out


def table_line(many, cap, conds, programs):
    parts = ["T", str(int(many)), str(cap), str(len(conds))]
    for kind, field, pat in conds:
        parts += [str(kind), hx(field), hx(pat)]
    parts.append(str(len(programs)))
    for p in programs:
        parts += [str(len(p))] + [str(o) for o in p]
    return " ".join(parts)


def parse_table(ans):
    status, cond, n_rx, blob_bytes, n_est = ans[:5]
    est = ans[5: 5 + n_est]
    at = 5 + n_est
    n_users = ans[at]
    users = ans[at + 1: at + 1 + n_users]
    at += 1 + n_users
    in_blob = ans[at + 1: at + 1 + ans[at]]
    return dict(status=status, cond=cond, n_rx=n_rx, blob_bytes=blob_bytes, est=est, users=users, in_blob=in_blob)


def align4(v):
    return (v + 3) & ~3


def test_constants_are_the_calls_limits(driver, tmp_path):
    assert run(driver, tmp_path, ["C"])[0] == [16, SINGLE_CAP, MANY_CAP, 4, 4, 96]
    assert MANY_CAP == 80 * 1024 - 43780 and SINGLE_CAP - MANY_CAP == 6404


# ---- co_active_bound ----

def covers(a, path):
    return a != "" and (path == a or path.startswith(a + "."))


def brute_bound(fields):
    """the most conditions any path can lie under: every field, every field extended, and every dotted prefix of a field"""
    paths = set()
    for f in fields:
        parts = f.split(".")
        paths.update(".".join(parts[:i]) for i in range(1, len(parts) + 1))
        paths.update([f, f + ".zz", f + "x", f + ".", f + "..q"])
    return max((sum(covers(a, p) for a in fields) for p in paths), default=0)


def random_fields(rng, n):
    names = ["a", "b", "ab", "message", "user", "", "a.b"]
    out = []
    for _ in range(n):
        depth = int(rng.integers(1, 5))
        out.append(".".join(names[int(rng.integers(0, len(names)))] for _ in range(depth)))
    return out


def test_co_active_bound_is_the_brute_force_count(driver, tmp_path):
    rng = np.random.default_rng(20261016)
    sets = [[], ["a"], ["a", "a"], ["a", "ab"], ["a", "a.b", "a.b.c", "a.bc"], ["message"] * 6, ["", "", "a"], ["a.", "a", "a..b"],
            ["user", "user.name", "user.id", "users"], ["x.y", "x", "x.y.z", "x.y", "q"]]
    sets += [random_fields(rng, int(rng.integers(1, 17))) for _ in range(400)]
    got = run(driver, tmp_path, [" ".join(["B"] + [hx(f) for f in s]) for s in sets])
    seen = set()
    for s, g in zip(sets, got):
        assert g == [brute_bound(s)], s
        seen.add(g[0])
    assert got[2] == [2] and got[3] == [1] and got[4] == [3] and got[5] == [6] and got[6] == [1] and got[8] == [2] and got[9] == [4]
    assert {0, 1, 2, 3, 4, 5} <= seen          # below, at and above both slot counts


# ---- the byte estimate ----

def test_estimate_is_the_stated_formula(driver, tmp_path):
    cases = [(s, c, f, m) for s in (1, 2, 7, 1000, 1024) for c in (1, 2, 3, 17, 256) for f in (0, 1, 5, 96, 97, 300) for m in (0, 1)]
    got = run(driver, tmp_path, ["E %d %d %d %d" % c for c in cases])
    for (s, c, f, m), g in zip(cases, got):
        assert g == [16 + 8 * m + align4(256 + 2 * s * c) + (f if f <= 96 else 0)], (s, c, f, m)


def test_estimate_against_the_blob_of_the_regex_suites_patterns(driver, tmp_path):
    pats = py_patterns()
    assert len(pats) == 25
    sizes = run(driver, tmp_path, ["D " + hx(p) for p in pats])
    assert all(ok == 1 and s >= 1 and c >= 1 for ok, s, c in sizes)
    fields = ["message", "nested.region", "a", "日本語", "k" * 96, "k" * 97, "user.name"]
    lines, tables = [], []
    for many in (0, 1):
        for lo in range(0, len(pats), 5):
            for n in (1, 2, 7, 16):
                conds = [(_lib.KIND_FIELD_REGEX, fields[(lo + i) % len(fields)], pats[(lo + i) % len(pats)]) for i in range(n)]
                conds.insert(1, (_lib.KIND_FIELD_TOKEN, "level", "error"))          # a plain condition in between costs nothing
                tables.append((many, conds))
                lines.append(table_line(many, MANY_CAP if many else SINGLE_CAP, conds, [[_lib.op(_lib.OP_TERM, c) for c in range(len(conds))]]))
    for (many, conds), ans in zip(tables, run(driver, tmp_path, lines)):
        t = parse_table(ans)
        rx = [c for c in conds if c[0] == _lib.KIND_FIELD_REGEX]
        assert t["status"] == OK and t["n_rx"] == len(rx) == len(t["est"])
        for (_, field, pat), est in zip(rx, t["est"]):
            _, s, c = sizes[pats.index(pat)]
            flen = len(field.encode())
            assert est == 16 + 8 * many + align4(256 + 2 * s * c) + (flen if flen <= 96 else 0), (field, pat)
        total = align4(sum(t["est"]))
        # build_blob pads in front of a region: the padding behind the last one is not spent
        assert t["blob_bytes"] <= total <= t["blob_bytes"] + 4, (many, conds)


def counted(n_conds, reps):
    return [(_lib.KIND_FIELD_REGEX, "f%d" % i, "^[0-9a-f]{%d}$" % (reps + i)) for i in range(n_conds)]


def test_a_table_between_the_two_caps_by_the_estimate(driver, tmp_path):
    """nine ~1 000-state DFAs: over the batched call's 38 140 bytes, within the single call's 44 544 (the GPU suite uses this table)"""
    conds = counted(9, 991)
    prog = [[_lib.op(_lib.OP_TERM, c) for c in range(9)] + [_lib.op(_lib.OP_OR, 9)]]
    single, many, eight = [parse_table(a) for a in run(driver, tmp_path, [table_line(0, SINGLE_CAP, conds, prog), table_line(1, MANY_CAP, conds, prog),
                                                                           table_line(1, MANY_CAP, conds[:8], prog)])]
    assert single["status"] == OK and MANY_CAP < single["blob_bytes"] <= SINGLE_CAP
    assert MANY_CAP < align4(sum(single["est"])) + 8 * 9 <= SINGLE_CAP
    assert many["status"] == OVER_CAP and many["blob_bytes"] == 0
    assert eight["status"] == OK and eight["blob_bytes"] <= MANY_CAP and align4(sum(eight["est"])) <= MANY_CAP


def test_blob_refusals(driver, tmp_path):
    prog = [[_lib.op(_lib.OP_TERM, 0)]]
    seventeen = [(_lib.KIND_FIELD_REGEX, "f", "x%d" % i) for i in range(17)]
    outside = [(_lib.KIND_FIELD_TOKEN, "level", "error"), (_lib.KIND_FIELD_REGEX, "a", "x"), (_lib.KIND_FIELD_REGEX, "a", "\\bx")]
    none = [(_lib.KIND_FIELD_TOKEN, "level", "error")]
    a, b, c = [parse_table(x) for x in run(driver, tmp_path, [table_line(1, MANY_CAP, seventeen, prog), table_line(1, MANY_CAP, outside, prog),
                                                               table_line(1, MANY_CAP, none, prog)])]
    assert a["status"] == TOO_MANY and a["n_rx"] == 17
    assert b["status"] == PATTERN and b["cond"] == 2
    assert c["status"] == OK and c["n_rx"] == 0 and c["blob_bytes"] == 0


# ---- user masks ----

def test_user_masks_are_the_programs_references(driver, tmp_path):
    rng = np.random.default_rng(5)
    lines, batches = [], []
    for n_queries in (1, 2, 17, 64):
        pairs = []
        for q in range(n_queries):
            bloom = [None, Q.FieldToken("level", "error"), Q.Or(Q.Token("timeout"), Q.Field("nested.az"))][int(rng.integers(0, 3))]
            if q == n_queries - 1:
                bloom = Q.FieldToken("level", "error")                               # the last query references something: bit n - 1 is in use
            kids = [Q.FieldRegex("f%d" % int(rng.integers(0, 6)), "x%d" % int(rng.integers(0, 2))) for _ in range(int(rng.integers(0, 4)))]
            regex = None if not kids else kids[0] if len(kids) == 1 else Q.RegexOr(*kids)
            pairs.append((bloom, regex))
        b = Q.CompiledRowQueryBatch(pairs)
        batches.append(b)
        conds = list(zip(b.kinds, b.fields, b.tokens))
        lines.append(table_line(1, MANY_CAP, conds, [b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]] for q in range(b.n_queries)]))
    for b, ans in zip(batches, run(driver, tmp_path, lines)):
        t = parse_table(ans)
        want = [0] * len(b.kinds)
        for q in range(b.n_queries):
            for o in b.prog_ops[b.prog_off[q]: b.prog_off[q + 1]]:
                if o >> 28 == _lib.OP_TERM:
                    want[o & 0x0FFFFFFF] |= 1 << q
        assert t["status"] == OK and t["users"] == want
        assert all(want)                                                           # every table condition has a user
        # ... and the blob carries the regex conditions' masks, in slot order, behind its header
        assert t["in_blob"] == [want[c] for c in range(len(b.kinds)) if b.kinds[c] == _lib.KIND_FIELD_REGEX]
    assert batches[-1].n_queries == 64 and any(u >> 63 for u in t["users"])       # bit 63 is in use
