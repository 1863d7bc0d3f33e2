"""The row matcher's route on the CPU (no GPU): tests/match_route_check.cpp drives bloomsearch_amd/csrc/host/match_route.hpp — the
header csrc/match_api.inc reads every call's refusals, tables, LDS cap, walker and trace name from — built twice with g++: plain with
-Wall -Wextra -Werror, and under AddressSanitizer and UBSan.

Reference: `expected` below, the route restated call by call from the table in DESIGN.md ("Row matcher: the route"), not from the
header.  For every call spec, every table over the kind classes {0-2, 3, 4, 5, 6, 7} of length 0 to 3 in every order (so the condition
a refusal names is checked), and a 64-condition table per consumer set; the batched calls with 0 and with 3 queries.  Compared: the
status, on a refusal which one, the condition and its kind, else each build flag, the cap, the consumer set and the trace name.
The walker list (the X-macro the launch table is made of) is read back as strings: 60 slots each filled once, the lookup mode with
the none and regex sets only, every kernel named after its (mode, set, tokenizer)."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "match_route_check.cpp")

MODES = ("Single", "Many", "Wide", "Lookup")
SETS = ("None", "Regex", "Substr", "RegexSubstr", "Range", "RegexSubstrRange")
TOKS = ("Default", "Spec", "Gram")
MODE_PART = {"Single": "", "Many": "_many", "Wide": "_store", "Lookup": "_lookup"}
SET_PART = {"None": "", "Regex": "_regex", "Substr": "_substr", "RegexSubstr": "_regex_substr", "Range": "_range", "RegexSubstrRange": "_regex_substr_range"}
TOK_PART = {"Default": "", "Spec": "_tok", "Gram": "_gram"}

# entry point -> (mode, the family its row of the route table belongs to, policy, trace name, trace name without a regex condition)
SPECS = {}
for mode, prefix in (("Single", "bsg_match_rows"), ("Many", "bsg_match_rows_many")):
    for suffix, family in (("", "plain"), ("_regex", "regex"), ("_substr", "substr"), ("_range", "range"), ("_regex_substr", "regex_substr"),
                           ("_regex_substr_range", "all")):
        SPECS[prefix + suffix] = (mode, family, "Bits", prefix + suffix, prefix + suffix)
SPECS["bsg_match_rows_tok"] = ("Single", "regex", "Bits", "bsg_match_rows", "bsg_match_rows")
SPECS["bsg_match_rows_regex"] = ("Single", "regex", "Bits", "bsg_match_rows", "bsg_match_rows")
SPECS["bsg_match_rows_many_regex"] = ("Many", "regex", "Bits", "bsg_match_rows_many_regex", "bsg_match_rows_many")
for suffix, family in (("", "regex"), ("_substr", "regex_substr"), ("_range", "range"), ("_regex_substr_range", "all")):
    for tail, policy in (("", "Bits"), ("_rows", "Rows")):
        SPECS["bsg_match_rows_wide" + suffix + tail] = ("Wide", family, policy, "bsg_match_rows_wide" + suffix + tail, "bsg_match_rows_wide" + suffix + tail)
SPECS["bsg_match_rows_wide_hist"] = ("Wide", "all", "Hist", "bsg_match_rows_wide_hist", "bsg_match_rows_wide_hist")
for suffix, family in (("", "plain"), ("_regex", "regex")):
    for tail, policy in (("", "Bits"), ("_rows", "Rows")):
        SPECS["bsg_match_rows_lookup" + suffix + tail] = ("Lookup", family, policy, "bsg_match_rows_lookup" + suffix + tail, "bsg_match_rows_lookup" + suffix + tail)
ACCEPTS = {"plain": "Plain", "regex": "Regex", "substr": "Substr", "range": "Range", "regex_substr": "RegexSubstr", "all": "All"}
CAPS = {"Single": ("Single", "SingleSub"), "Many": ("Many", "ManySub"), "Wide": ("Wide", "WideSub"), "Lookup": ("Lookup", None)}


def first(kinds, pred):
    return next(((c, k) for c, k in enumerate(kinds) if pred(k)), None)


def expected(name, kinds, n_queries):
    """The route table, row by row.  A refusal: (status, refusal, cond, kind); else a dict of what is built."""
    mode, family, _, trace, trace_plain = SPECS[name]
    R, S, N = 3 in kinds, 4 in kinds or 5 in kinds, 6 in kinds
    refusal = None
    if family == "all":                                  # kind > 6, found by a scan of the whole table before any other check
        bad = first(kinds, lambda k: k > 6)
        if bad:
            return ("Invalid", "UnknownKind") + bad
        family = "regex_substr" if not N else "range" if not (R or S) else "three"
    elif family == "plain" and mode == "Lookup":          # kind > 3 unknown; kind 3 passes the route: build_strings refuses it by name
        bad = first(kinds, lambda k: k > 3)
        if bad:
            return ("Invalid", "UnknownKind") + bad
    else:                                                # per condition: regex-with-substr, text-with-range, (batched regex), unknown kind
        for c, k in enumerate(kinds):
            if family == "substr" and k == 3:
                refusal = ("Unsupported", "RegexWithSubstr", c, k)
            elif family == "range" and 3 <= k <= 5:
                refusal = ("Unsupported", "TextWithRange", c, k)
            elif family == "plain" and mode == "Many" and k == 3:
                refusal = ("Unsupported", "RegexInBatched", c, k)
            elif k > {"plain": 2, "regex": 3, "substr": 5, "range": 6, "regex_substr": 5}[family]:
                refusal = ("Invalid", "UnknownKind", c, k)
            if refusal:
                return refusal
    cap, cap_sub = CAPS[mode]
    many = mode == "Many"
    out = {"blob": False, "cap": "None", "users": False, "needles": False, "range": False, "set": "None", "trace": trace if R else trace_plain}
    if family == "regex":                                # the batched blob only when there is a query
        out.update(blob=not many or n_queries > 0, cap=cap, set="Regex" if R else "None")
    elif family == "substr":                             # needle tables always; substr walker always
        out.update(needles=True, set="Substr")
    elif family == "range":
        out.update(range=True, set="Range" if N else "None")
    elif family == "regex_substr":                       # the cap beside a needle table iff S; needles iff S; walker by (R, S)
        out.update(blob=not many or n_queries > 0, cap=cap_sub if S else cap, needles=S,
                   set={(False, False): "None", (True, False): "Regex", (False, True): "Substr", (True, True): "RegexSubstr"}[(R, S)])
    elif family == "three":                              # built either way, needle or not
        out.update(blob=True, cap=cap_sub, needles=True, range=True, set="RegexSubstrRange")
    if not out["blob"]:
        out["cap"] = "None"
    out["users"] = many and out["blob"]
    return out


def tables():
    """every table of length 0 to 3 over a member of each kind class, every order; one 64-condition table per consumer set"""
    classes = (1, 3, 4, 5, 6, 7)
    out = [list(t) for n in range(4) for t in itertools.product(classes, repeat=n)]
    assert len(out) == 259
    for mix in ((0, 1, 2), (3, 0), (4, 2, 5), (3, 4, 1), (6, 0, 2), (6, 3, 5, 1)):
        out.append([mix[i % len(mix)] for i in range(64)])
    out += [[0, 2, 0], [2, 7, 3], [0, 0xFFFFFFFF]]       # the other plain kinds, and a kind far past the known ones
    return out


def build(dirname, flags):
    exe = os.path.join(str(dirname), "match_route_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", exe, SRC],
                   check=True, timeout=300)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return build(tmp_path_factory.mktemp("match_route_" + request.param), flags)


def run(exe, tmp_path, cases):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-6000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) - 1 == len(cases)
    return got[:-1]


def test_every_entry_point_has_its_spec(exe, tmp_path):
    got = [s.split(":") for s in run(exe, tmp_path, ["specs"])[0].split()]
    assert len(got) == len(SPECS) == 26 and {g[0] for g in got} == set(SPECS)
    for name, mode, accepts, policy in got:
        assert (mode, accepts, policy) == (SPECS[name][0], ACCEPTS[SPECS[name][1]], SPECS[name][2]), name


def test_route_of_every_spec_over_every_small_table(exe, tmp_path):
    names = [s.split(":")[0] for s in run(exe, tmp_path, ["specs"])[0].split()]
    cases, want = [], []
    for i, name in enumerate(names):
        for kinds in tables():
            for n_queries in ((0, 3) if SPECS[name][0] == "Many" else (1,)):
                cases.append("route %d %d %d %s" % (i, n_queries, len(kinds), " ".join(map(str, kinds))))
                want.append((name, kinds, n_queries))
    seen = set()
    for line, case, (name, kinds, n_queries) in zip(run(exe, tmp_path, cases), cases, want):
        status, refusal, cond, kind, blob, cap, users, needles, rng, cset, trace = line.split()
        e = expected(name, kinds, n_queries)
        if isinstance(e, tuple):
            assert (status, refusal, int(cond), int(kind)) == e, (name, case, line)
            seen.add(refusal)
            continue
        got = {"blob": blob == "1", "cap": cap, "users": users == "1", "needles": needles == "1", "range": rng == "1", "set": cset, "trace": trace}
        assert (status, refusal) == ("Ok", "None") and got == e, (name, case, line, e)
        seen.add((SPECS[name][0], cset))
    assert {"UnknownKind", "RegexWithSubstr", "TextWithRange", "RegexInBatched"} <= seen
    routed = {s for s in seen if isinstance(s, tuple)}                   # every walker family is reached by some call
    assert routed == {(m, c) for m in MODES for c in SETS if m != "Lookup" or c in ("None", "Regex")}


def test_the_walker_list_fills_every_slot_once(exe, tmp_path):
    walkers, slots = run(exe, tmp_path, ["walkers", "slots"])
    slots = [int(x) for x in slots.split()]
    assert slots[0] == 60 and len(slots) == 1 + 4 * 6 * 3
    by_key = dict(zip(itertools.product(MODES, SETS, TOKS), slots[1:]))
    valid = {k: v for k, v in by_key.items() if k[0] != "Lookup" or k[1] in ("None", "Regex")}
    assert sorted(valid.values()) == list(range(60)) and all(v == -1 for k, v in by_key.items() if k not in valid)
    lines = [w.split(":") for w in walkers.split()]
    assert len(lines) == 60
    filled = {}
    for mode, cset, tok, kernel, at in lines:
        assert (mode, cset, tok) in valid and int(at) == valid[(mode, cset, tok)] and int(at) not in filled, (mode, cset, tok, kernel)
        assert kernel == "k_match_rows" + MODE_PART[mode] + SET_PART[cset] + TOK_PART[tok], (mode, cset, tok, kernel)
        filled[int(at)] = kernel
    assert sorted(filled) == list(range(60)) and len(set(filled.values())) == 60
    assert {c for m, c, _, _, _ in lines if m == "Lookup"} == {"None", "Regex"}
