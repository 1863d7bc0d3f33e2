"""What the tests of bsg_match_rows_regex_substr_range / bsg_match_rows_many_regex_substr_range share: the expected verdict of a
(bloom, regex, substring, range) query on a row from the four restatements the suite already has (none asks the library), the
Python `re` spellings of the patterns these tests add, an evaluator of public programs over per-condition verdicts, and the rows and
literal bits of the edge cases.  Test infrastructure only: nothing below touches the GPU."""
import json
import os
import re

import numpy as np

from bloomsearch_amd import query as Q
from bloomsearch_amd._lib import OP_AND, OP_OR, OP_TERM, op
from tests import ngram_restatement as NR
from tests import range_restatement as RR
from tests import substring_restatement as SR
from tests.test_match_regex_gpu import PY, oracle_row

WALKERS = sorted(SR.WALKERS)
SINGLE_CAP, MANY_CAP = 40448, 34032              # match.hip.h kRxSubLdsCap, kRxManySubLdsCap: the caps beside a needle table

# patterns beside test_match_regex_gpu.PY, each with the same language spelled for Python `re`
EXTRA = {"^17": "\\A17", "^5$": "\\A5\\Z", "out$": "out\\Z", "^12$": "\\A12\\Z", "2": "2", "^1$": "\\A1\\Z", "timeout": "timeout", "timeout$": "timeout\\Z",
         "x$": "x\\Z", "^x": "\\Ax", "^x$": "\\Ax\\Z", "^w": "\\Aw", "^e": "\\Ae", "^1": "\\A1"}
COUNTED = re.compile(r"\^\[0-9a-f\]\{(\d+)\}\$")


def py_runner(pattern, text):
    m = COUNTED.fullmatch(pattern)
    if m:
        return re.search("\\A[0-9a-f]{%s}\\Z" % m.group(1), text) is not None
    return re.search(PY[pattern] if pattern in PY else EXTRA[pattern], text) is not None


def verdict(r, bloom, regex, sub, rng, tok):
    return bool(NR.row_verdict(r, SR.spec_of(tok), bloom, None) and oracle_row(r, None, regex, py_runner) and SR.row_verdict(r, sub, tok) and
                RR.row_verdict(r, rng))


def want(rows, bloom, regex, sub, rng, tok):
    return np.array([verdict(r, bloom, regex, sub, rng, tok) for r in rows], dtype=bool)


def row(**kv):
    return json.dumps(kv, ensure_ascii=False, separators=(",", ":")).encode()


T = lambda c: op(OP_TERM, c)
AND = lambda n: op(OP_AND, n)
OR = lambda n: op(OP_OR, n)


def table(regexes, subs, ranges, blooms=()):
    """ONE table: the bloom conditions first, then the regex, the substring and the range ones (CompiledRowTextRangeQuery's order)
    -> (matcher, [the verdict function of condition c])"""
    m = Q.CompiledRowTextRangeQuery(Q.And(*blooms) if blooms else None, Q.RegexAnd(*regexes), Q.SubstringAnd(*subs), Q.RangeAnd(*ranges))
    assert len(m.kinds) == len(blooms) + len(regexes) + len(subs) + len(ranges)
    sides = [(b, None, None, None) for b in blooms] + [(None, r, None, None) for r in regexes] + [(None, None, s, None) for s in subs] + \
            [(None, None, None, g) for g in ranges]
    return m, sides


def sat_columns(rows, sides, tok):
    return [want(rows, *s, tok) for s in sides]


def evaluate(prog, sat):
    """a public postfix program over per-condition verdict columns"""
    stack = []
    for o in prog:
        opc, arg = o >> 28, o & 0x0FFFFFFF
        if opc == OP_TERM:
            stack.append(sat[arg])
        else:
            kids, stack = stack[len(stack) - arg:], stack[:len(stack) - arg]
            stack.append(np.logical_and.reduce(kids) if opc == OP_AND else np.logical_or.reduce(kids))
    return stack[0]


def unassigned_rune() -> str:
    """a rune the device's lower table cannot decide: the first code point of the committed list"""
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unicode13_unassigned.json")))
    first = g["ranges"][0]
    return chr(first[0] if isinstance(first, (list, tuple)) else first)


DEEP17 = b'{"a":' * 17 + b'5' + b'}' * 17 + b''    # seventeen containers open at once: outside the walker's envelope

# ---- edge cases: (name, rows, regexes, substrings, ranges, [(program, literal bits)]) over the table regexes + substrings + ranges ----
I64_MAX = (1 << 63) - 1
EDGES = [
    ("one number leaf read by all three consumers",
     [b'{"ts":1700000123}', b'{"ts":1700000124}', b'{"ts":"1700000123"}', b'{"ts":2700000123}'],
     [Q.FieldRegex("ts", "^17")], [Q.Substring("00123")], [Q.FieldRange("ts", 1700000000, 1700000200)],
     [([T(0)], [1, 1, 1, 0]), ([T(1)], [1, 0, 1, 1]), ([T(2)], [1, 1, 0, 0]), ([T(0), T(1), T(2), AND(3)], [1, 0, 0, 0]),
      ([T(0), T(1), T(2), OR(3)], [1, 1, 1, 1])]),
    ("a string never holds for a range condition, and the needle has no carry between two leaves",
     [b'{"a":12,"b":"12"}', b'{"a":1,"b":"2"}', b'{"a":"12","b":12}'],
     [Q.FieldRegex("b", "^12$")], [Q.Substring("12"), Q.Substring("1212"), Q.FieldSubstring("b", "12")], [Q.FieldRange("b", 12, 12), Q.FieldRange("a", 12, 12)],
     [([T(0)], [1, 0, 1]), ([T(1)], [1, 0, 1]), ([T(2)], [0, 0, 0]), ([T(3)], [1, 0, 1]), ([T(4)], [0, 0, 1]), ([T(5)], [1, 0, 0]),
      ([T(0), T(1), T(4), AND(3)], [0, 0, 1])]),
    ("a number as the row's last leaf: decided after the walk",
     [b'{"s":"t","n":5}', b'{"s":"t","n":55}', b'{"n":5}', b'{"s":"t","n":5 }', b'{"s":"5","n":6}'],
     [Q.FieldRegex("n", "^5$")], [Q.FieldSubstring("n", "5")], [Q.FieldRange("n", 5, 5)],
     [([T(0)], [1, 0, 1, 1, 0]), ([T(1)], [1, 1, 1, 1, 0]), ([T(2)], [1, 0, 1, 1, 0]), ([T(0), T(1), T(2), AND(3)], [1, 0, 1, 1, 0])]),
    ("array elements are leaves of the array's path",
     [b'{"v":[1,"timeout",30]}', b'{"v":[1,"timeout",31]}', b'{"v":[30,"timeouts"]}', b'{"v":[1,"time","out",3,0]}'],
     [Q.FieldRegex("v", "out$")], [Q.FieldSubstring("v", "timeout")], [Q.FieldRange("v", 30, 30)],
     [([T(0)], [1, 1, 0, 1]), ([T(1)], [1, 1, 1, 0]), ([T(2)], [1, 0, 1, 0]), ([T(0), T(1), T(2), AND(3)], [1, 0, 0, 0])]),
    ("none of the three consumers sees a pathless leaf",
     [b'{"a":1,"":2}', b'{"a":12}', b'{"a":2}'],
     [Q.FieldRegex("a", "2"), Q.FieldRegex("a", "^1$")], [Q.Substring("2"), Q.Substring("12")],
     [Q.FieldRange("a", 2, 2), Q.FieldRange("a", 12, 12), Q.FieldRange("a", 1, 1)],
     [([T(0)], [0, 1, 1]), ([T(1)], [1, 0, 0]), ([T(2)], [0, 1, 1]), ([T(3)], [0, 1, 0]), ([T(4)], [0, 0, 1]), ([T(5)], [0, 1, 0]), ([T(6)], [1, 0, 0])]),
    ("literals a float64 would bend, beside needles that match their text",
     [b'{"v":-0.0}', b'{"v":5.000}', ('{"v":%s}' % RR.BIG).encode(), b'{"v":9007199254740993}'],
     [Q.FieldRegex("v", "^-?[0-9]+(\\.[0-9]+)?$")], [Q.Substring("-0.0"), Q.Substring("5.000"), Q.Substring(RR.BIG[10:30]), Q.Substring("40993")],
     [Q.FieldRange("v", 0, 0), Q.FieldRange("v", 5, 5), Q.FieldRange("v", None, I64_MAX), Q.FieldRange("v", I64_MAX, None),
      Q.FieldRange("v", 9007199254740993, 9007199254740993), Q.FieldRange("v", 9007199254740992, 9007199254740992)],
     [([T(0)], [1, 1, 1, 1]), ([T(1)], [1, 0, 0, 0]), ([T(2)], [0, 1, 0, 0]), ([T(3)], [0, 0, 1, 0]), ([T(4)], [0, 0, 0, 1]),
      ([T(5)], [1, 0, 0, 0]), ([T(6)], [0, 1, 0, 0]), ([T(7)], [1, 1, 0, 1]), ([T(8)], [0, 0, 1, 0]), ([T(9)], [0, 0, 0, 1]), ([T(10)], [0, 0, 0, 0])]),
]


def check_edges_against_the_restatements(tok=None):
    """the literal bits above ARE what the restatements say (run on the CPU by tests/test_range_text_cabi.py)"""
    for name, rows, rxs, sxs, rgs, progs in EDGES:
        _, sides = table(rxs, sxs, rgs)
        sat = sat_columns(rows, sides, tok)
        for prog, bits in progs:
            assert evaluate(prog, sat).tolist() == [bool(b) for b in bits], (name, prog, evaluate(prog, sat).tolist())


# ---- the 64-condition table: 16 tokens, 16 regex conditions, 16 needles of 8 bytes (128 packed bytes), 16 ranges ----
def full_table():
    blooms = [Q.Token("w%02d" % j) for j in range(16)]                       # 3 runes: one window of the trigram walker too
    regexes = [Q.FieldRegex("r%d" % j, "^[0-9a-f]{%d}$" % (j + 1)) for j in range(16)]
    subs = [Q.Substring("n%02d-abcd" % j) if j % 2 == 0 else Q.FieldSubstring("s", "n%02d-abcd" % j) for j in range(16)]
    ranges = [Q.FieldRange("n%d" % j, 100 * j, 100 * j + 1) for j in range(16)]
    rows = []
    for i in range(48):
        j, k = i % 16, i // 16
        rows.append(row(t="zz w%02d zz" % ((j + 2 * k) % 16), s="zz n%02d-abcd zz" % ((j + k) % 16), **{"r%d" % j: "a" * (j + 1 + (k == 1)), "n%d" % j: 100 * j + k}))
    return rows, blooms, regexes, subs, ranges
