"""A restatement of the range conditions (include/bloomgpu.h "Range conditions") in plain Python, for the tests of host/range.hpp and of
the device walkers: rows are parsed by json.loads with hooks that see every number's RAW literal and turn it into an exact Fraction,
every pair of an object is kept (duplicate keys too), and a walk yields (path, value) for the number leaves as the row walker names
them.  No float is involved anywhere."""
import decimal
import fractions
import json

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = "1234567890123456789012345678901234567890"                # 40 digits

LITERALS = [
    "0", "-0", "-0.0", "5", "5.000", "5.0001", "-5.5", "0.999999999999999999999", "-5", "-6", "4.9999999999999999999", "-0.5", "6", "1", "-1",
    "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "9223372036854775806.5",
    "-9223372036854775808.0000000000000000001", "9223372036854775807.0", "-9223372036854775807",
    "18446744073709551615", "18446744073709551616", "18446744073709551615.5", "-18446744073709551616", BIG, "-" + BIG, BIG + ".5",
    "9" * 20,                                                   # past 2^64
    "1e3", "1E+21", "2.5e-7", "-1e-400", "123456789e-3", "5e0", "0e5", "-0.0e-3", "9223372036854775807e0", "92233720368547758070e-1", "1e400",
]
PLAIN_LITERALS = [s for s in LITERALS if "e" not in s and "E" not in s]

# a bound: None (absent) or (value, open)
BOUND_VALUES = [I64_MIN, I64_MIN + 1, -6, -5, -1, 0, 1, 5, 6, I64_MAX - 1, I64_MAX]
BOUNDS = [None] + [(v, o) for v in BOUND_VALUES for o in (False, True)]
BOUND_PAIRS = [(lo, hi) for lo in BOUNDS for hi in BOUNDS]


def exact(literal: str) -> fractions.Fraction:
    return fractions.Fraction(decimal.Decimal(literal))


class Obj:
    def __init__(self, pairs):
        self.pairs = pairs


def parse(row: bytes):
    return json.loads(row, parse_int=exact, parse_float=exact, object_pairs_hook=Obj)


def number_leaves(node, path=""):
    """(path, value) of every number leaf that has a path; an array's elements lie under the array's path"""
    if isinstance(node, Obj):
        for k, v in node.pairs:
            yield from number_leaves(v, (path + "." if path else "") + k)
    elif isinstance(node, list):
        for v in node:
            yield from number_leaves(v, path)
    elif isinstance(node, fractions.Fraction) and path:
        yield path, node


def inside(value, lo, hi) -> bool:
    """lo / hi: None or (int, open)"""
    if lo is not None and (value <= lo[0] if lo[1] else value < lo[0]):
        return False
    if hi is not None and (value >= hi[0] if hi[1] else value > hi[0]):
        return False
    return True


def field_range(Q, field, lo, hi):
    """query.FieldRange from a pair of bounds"""
    return Q.FieldRange(field, None if lo is None else lo[0], None if hi is None else hi[0], lo_open=bool(lo and lo[1]), hi_open=bool(hi and hi[1]))


def condition_holds(cond: dict, leaves) -> bool:
    field = cond.get("Field", "")
    lo = None if cond.get("Lo") is None else (cond["Lo"], bool(cond.get("LoOpen")))
    hi = None if cond.get("Hi") is None else (cond["Hi"], bool(cond.get("HiOpen")))
    return field != "" and any(p == field and inside(v, lo, hi) for p, v in leaves)


def tree_holds(tree, leaves) -> bool:
    if tree is None:
        return True
    t = tree.get("ExpressionType")
    if t == "CONDITION":
        c = tree.get("Condition")
        return True if c is None else condition_holds(c, leaves)
    kids = [tree_holds(c, leaves) for c in tree.get("Children") or []]
    return all(kids) if t == "AND" else any(kids) if t == "OR" else False


def row_verdict(row: bytes, tree) -> bool:
    return tree_holds(tree, list(number_leaves(parse(row))))


def P(v):
    """the closed point interval [v, v]"""
    return ((v, False), (v, False))


# Path and leaf rules: (row, [(field, (lo, hi), expected)])
KEY20 = "k" * 20
PATH_CASES = [
    (b'{"a":1,"":2}', [("a", P(12), False), ("a", P(1), True), ("a", P(2), False)]),          # the pathless 2 is not appended to a's 1
    (b'{"a":[1,2]}', [("a", P(12), False), ("a", P(1), True), ("a", P(2), True)]),            # each element is a leaf of its own
    (b'{"a":1,"b":2}', [("a", P(12), False), ("a", P(1), True), ("b", P(2), True), ("a", P(2), False), ("b", P(1), False)]),
    (b'{"a":{"b":7}}', [("a.b", P(7), True), ("a", P(7), False), ("b", P(7), False)]),         # equality, not "at or beneath"
    (b'{"a.b":7}', [("a.b", P(7), True), ("a", P(7), False)]),
    (b'{"a":"5"}', [("a", P(5), False), ("a", (None, None), False)]),                         # strings never hold
    (b'{"a":true}', [("a", (None, None), False)]),
    (b'{"a":null}', [("a", (None, None), False)]),
    (b'{"a":5,"a":9}', [("a", P(5), True), ("a", P(9), True), ("a", P(59), False)]),           # both leaves count
    (b'{"x":"9","a":5}', [("a", P(5), True), ("a", P(9), False), ("a", P(95), False), ("x", (None, None), False)]),
    (b'{"s":"t","a":-17}', [("a", P(-17), True), ("a", P(17), False)]),                       # the row's last value
    (b'{"a":42 ,"b": 7 }', [("a", P(42), True), ("b", P(7), True), ("a", P(427), False)]),     # a number followed by a space
    (('{"%s":123456}' % KEY20).encode(), [(KEY20, P(123456), True), (KEY20[:19], P(123456), False)]),
    (b'{"a":[{"b":3},4,[5]],"c":{"":6,"d":[]}}', [("a.b", P(3), True), ("a", P(4), True), ("a", P(5), True), ("a", P(3), False), ("c.", P(6), True), ("c", P(6), False)]),
    (b'7', [("", (None, None), False)]),                                                      # a scalar at the root has no path
    (b'{"":7}', [("", (None, None), False), ("", P(7), False)]),                              # an empty field never holds
] + [(('{"%s":%d,"z":1}' % ("k" * (1 + s), 1000 + s)).encode(), [("k" * (1 + s), P(1000 + s), True), ("k" * (1 + s), P(1), False), ("z", P(1), True)])
     for s in range(9)]                                                                       # a key at each alignment to an 8-byte scan step
