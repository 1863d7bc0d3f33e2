"""Named rows for the MinMax index (include/bloomgpu.h "per-set MinMax indexes"), each with the contribution it is expected to make,
and the batches the device tests run.  tests/test_minmax_shapes.py holds every expectation stated here against the restatement
(tests/minmax_restatement.py), so the GPU tests can rely on either."""
from tests.minmax_restatement import BIG, I64_MAX, I64_MIN

NAME64 = "n" * 64
FIELDS = ["ts", "a.b", NAME64]                 # the fields every shape is scanned with


class Shape:
    def __init__(self, name, row, want=None, undecided=False):
        """want: {field: (min, max)} the row contributes (by the contract: what the HOST function gives for every row, and the device
        for a row it decides); undecided: the device must hand the row back (it then contributes nothing on the device)."""
        self.name, self.row, self.want, self.undecided = name, row if isinstance(row, bytes) else row.encode(), want or {}, undecided

    def __repr__(self):
        return "Shape(%s)" % self.name


def _ts(lit, mn, mx, **kw):
    return [Shape("ts=%s alone" % lit[:24], '{"ts":%s}' % lit, {"ts": (mn, mx)}, **kw),
            Shape("ts=%s among members" % lit[:24], '{"level":"info","ts":%s,"msg":"hello world","n":{"x":1}}' % lit, {"ts": (mn, mx)}, **kw)]


SHAPES = []
# ---- literals ----
for lit, mn, mx in [("0", 0, 0), ("-0", 0, 0), ("-0.0", 0, 0), ("5.000", 5, 5), ("5.0001", 5, 6), ("-5.0001", -6, -5), ("0." + "9" * 40, 0, 1),
                    ("9223372036854775807", I64_MAX, I64_MAX), ("9223372036854775808", I64_MAX, I64_MAX),
                    ("-9223372036854775808", I64_MIN, I64_MIN), ("-9223372036854775809", I64_MIN, I64_MIN),
                    ("18446744073709551615", I64_MAX, I64_MAX), ("18446744073709551616", I64_MAX, I64_MAX),
                    (BIG, I64_MAX, I64_MAX), ("-" + BIG, I64_MIN, I64_MIN),
                    ("9223372036854775806.5", I64_MAX - 1, I64_MAX), ("9223372036854775807.5", I64_MAX, I64_MAX),
                    ("-9223372036854775807.5", I64_MIN, I64_MIN + 1), ("-0.5", -1, 0), ("0.5", 0, 1), ("-17", -17, -17), ("1700000000", 1700000000, 1700000000)]:
    SHAPES += _ts(lit, mn, mx)
# an exponent on a field hands the row back (the host decides it exactly); on another key it changes nothing
for lit, mn, mx in [("1e3", 1000, 1000), ("1E+21", I64_MAX, I64_MAX), ("2.5e-7", 0, 1)]:
    SHAPES += _ts(lit, mn, mx, undecided=True)
    SHAPES.append(Shape("other=%s" % lit, '{"other":%s,"ts":7}' % lit, {"ts": (7, 7)}))
    SHAPES.append(Shape("nested ts=%s" % lit, '{"n":{"ts":%s},"ts":8}' % lit, {"ts": (8, 8)}))
# ---- values that are not numbers ----
for v in ['"5"', "true", "false", "null", "[5]", '{"x":5}']:
    SHAPES.append(Shape("ts=%s" % v, '{"ts":%s,"q":1}' % v, {}))
# ---- keys ----
SHAPES += [
    Shape("field first", '{"ts":1,"b":2,"c":3}', {"ts": (1, 1)}),
    Shape("field in the middle", '{"b":2,"ts":3,"c":4}', {"ts": (3, 3)}),
    Shape("field last", '{"b":2,"c":3,"ts":4}', {"ts": (4, 4)}),
    Shape("the key only nested", '{"n":{"ts":9}}', {}),
    Shape("the key nested in an array", '{"n":[{"ts":9},{"ts":10}]}', {}),
    Shape("top-level a.b", '{"a.b":1}', {"a.b": (1, 1)}),
    Shape("nested a -> b", '{"a":{"b":1}}', {}),
    Shape("both a.b forms", '{"a":{"b":1},"a.b":2}', {"a.b": (2, 2)}),
    Shape("t, ts, tsx", '{"t":1,"ts":2,"tsx":3}', {"ts": (2, 2)}),
    Shape("t and tsx only", '{"t":1,"tsx":3,"Ts":4,"s":5,"":6}', {}),
    Shape("the 64-byte name", '{"%s":64}' % NAME64, {NAME64: (64, 64)}),
    Shape("a 65-byte key", '{"%s":65}' % (NAME64 + "n"), {}),
    Shape("a 63-byte key", '{"%s":63}' % NAME64[:63], {}),
    Shape("65 then 64", '{"%s":65,"%s":-64}' % (NAME64 + "n", NAME64), {NAME64: (-64, -64)}),
    Shape("duplicated twice", '{"ts":1,"ts":5}', {"ts": (5, 5)}),
    Shape("duplicated twice, smaller last", '{"ts":5,"x":0,"ts":1}', {"ts": (1, 1)}),
    Shape("duplicated three times", '{"ts":1,"ts":9,"ts":-3.5}', {"ts": (-4, -3)}),
    Shape("duplicated, a string last", '{"ts":1,"ts":"x"}', {}),
    Shape("duplicated, null last", '{"ts":1,"ts":2,"ts":null}', {}),
    Shape("duplicated, an object last", '{"ts":1,"ts":{"ts":2}}', {}),
    Shape("duplicated, a number after a string", '{"ts":"x","ts":2}', {"ts": (2, 2)}),
    Shape("all three fields", '{"ts":-1,"a.b":2.5,"%s":3}' % NAME64, {"ts": (-1, -1), "a.b": (2, 3), NAME64: (3, 3)}),
    Shape("an escaped key that is the field", '{"t\\u0073":5}', {"ts": (5, 5)}, undecided=True),
    Shape("an escaped key that is no field", '{"x\\u0073":5,"ts":6}', {"ts": (6, 6)}, undecided=True),
    Shape("an escaped quote in a key", '{"t\\"s":5,"ts":6}', {"ts": (6, 6)}, undecided=True),
    Shape("an escaped key only nested", '{"n":{"t\\u0073":5},"ts":6}', {"ts": (6, 6)}),
]
# ---- strings that try to fool the scanner ----
SHAPES += [
    Shape("a value that looks like a member", '{"m":"\\"ts\\":5","ts":6}', {"ts": (6, 6)}),
    Shape("a value that looks like a member, no field", '{"m":"\\"ts\\":5"}', {}),
    Shape("a value of braces", '{"m":"}{","ts":7}', {"ts": (7, 7)}),
    Shape("a value of brackets and commas", '{"m":"],[,\\"ts\\":1,","ts":7}', {"ts": (7, 7)}),
    Shape("a value ending in an escaped backslash", '{"m":"x\\\\","ts":8}', {"ts": (8, 8)}),
    Shape("a value of two escaped backslashes and a quote", '{"m":"\\\\\\\\\\"","ts":8}', {"ts": (8, 8)}),
    Shape("a 300-byte string", '{"m":"%s","ts":9}' % ("ts\\\":1, " * 30 + "x" * 70), {"ts": (9, 9)}),
    Shape("a key named like a value", '{"5":"ts","ts":10}', {"ts": (10, 10)}),
]
# ---- structure ----
SHAPES += [
    Shape("nesting 40 deep", '{"d":' + '{"ts":' * 39 + "1" + "}" * 39 + ',"ts":11}', {"ts": (11, 11)}),
    Shape("arrays 40 deep", '{"d":' + "[" * 40 + '{"ts":1}' + "]" * 40 + ',"ts":12}', {"ts": (12, 12)}),
    Shape("whitespace everywhere", '  { "b" : 1 ,\t"ts"\n:\r\n 13.5 , "c" : [ 1 , 2 ] }  ', {"ts": (13, 14)}),
    Shape("whitespace before the closing brace", '{"ts":14 }', {"ts": (14, 14)}),
    Shape("an empty object", "{}", {}),
    Shape("empty containers", '{"a":{},"b":[],"ts":15}', {"ts": (15, 15)}),
]
assert len({s.name for s in SHAPES}) == len(SHAPES)

DECIDED = [s for s in SHAPES if not s.undecided]
UNDECIDED = [s for s in SHAPES if s.undecided]

# rows that are not valid JSON objects: inputs at the edge, whose set's result is unspecified
MALFORMED = [b'{"ts":5', b'{"ts":', b'{"ts"', b'{"t', b"{", b"", b"[1,2]", b"7", b'"ts"', b'{"ts":5}}', b'{"ts":5,', b'{"ts":"5', b'{"ts":5e}', b'{"m":"\\']


def synth_row(i: int) -> bytes:
    """an ordinary log row: ts spread over positive and negative values, some fractions"""
    ts = (i * 7919) % 100003 - 50000
    frac = ".%d" % (i % 10) if i % 3 == 0 else ""
    return ('{"id":%d,"level":"%s","ts":%d%s,"msg":"request %d served in %d ms","a.b":%d}' % (i, ("info", "warn", "error")[i % 3], ts, frac, i, i % 97, i % 11)).encode()


def size_rows(n: int):
    """n rows: the synthetic rows with every shape mixed in at a fixed stride"""
    rows = []
    for i in range(n):
        rows.append(SHAPES[(i // 5) % len(SHAPES)].row if i % 5 == 4 else synth_row(i))
    return rows


EIGHT = ["f%d" % i for i in range(8)]


def batches():
    """-> [(name, row_sets, fields)]"""
    out = []
    for n in (1, 63, 64, 65, 513):
        out.append(("one set of %d" % n, [size_rows(n)], FIELDS))
    out.append(("every shape its own set", [[s.row] for s in SHAPES], FIELDS))
    out.append(("every shape in one set", [[s.row for s in SHAPES]], FIELDS))
    out.append(("an empty set between two others", [size_rows(70), [], size_rows(3)], FIELDS))
    out.append(("a set without the key", [size_rows(10), [b'{"x":1}', b'{"y":{"ts":2}}', b'{"tsx":3}'] * 30, size_rows(5)], FIELDS))
    out.append(("a set where every row is handed back", [size_rows(66), [s.row for s in UNDECIDED] * 8, size_rows(2)], FIELDS))
    out.append(("eight fields, hits on the first and the eighth",
                [[('{"f0":%d,"f7":%d,"f8":1,"f":2}' % (i - 40, 1000 - i)).encode() for i in range(130)], [b'{"f7":-7.5}', b'{"f3":"x"}']], EIGHT))
    return out


def undecided_rows(row_sets):
    """{(set, index in set)} of the rows the shapes name as undecided"""
    bad = {s.row for s in UNDECIDED}
    return {(si, ri) for si, rows in enumerate(row_sets) for ri, r in enumerate(rows) if r in bad}
