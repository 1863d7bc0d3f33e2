"""Named cases for the bucket rule of bsg_match_rows_wide_hist: the MinMax shapes (tests/minmax_shapes.py, by import) under an ordinary
spec, and the bucket edges.  tests/test_hist_shapes.py holds every slot stated here against the restatement, so the GPU tests can rely
on either."""
from tests.hist_restatement import I64_MAX, I64_MIN
from tests.minmax_shapes import SHAPES, UNDECIDED, synth_row  # noqa: F401  (re-exported for the tests)

FIELD = "ts"
U64_MAX = (1 << 64) - 1


class Case:
    def __init__(self, name, row, origin, width, n_buckets, want=None, undecided=False, field=FIELD):
        """want: the slot by the contract (None: whatever the restatement says); undecided: the device hands the row back"""
        self.name, self.row = name, row if isinstance(row, bytes) else row.encode()
        self.origin, self.width, self.n_buckets, self.want, self.undecided, self.field = origin, width, n_buckets, want, undecided, field

    @property
    def spec(self):
        return self.field, self.origin, self.width, self.n_buckets

    def __repr__(self):
        return "Case(%s)" % self.name


def _ts(lit):
    return '{"level":"info","ts":%s,"msg":"m"}' % lit


CASES = []
# every MinMax shape under one ordinary spec: buckets of 3 from -10 on, 60 of them
for s in SHAPES:
    CASES.append(Case("shape: " + s.name, s.row, -10, 3, 60, undecided=s.undecided))
# ---- the edges of the buckets: origin 100, width 10, B buckets ----
for B in (1, 60, 1024):
    o, w = 100, 10
    edges = [(o - 1, B), (o, 0), (o + w - 1, 0), (o + w, 1 if B > 1 else B + 1), (o + B * w - 1, B - 1), (o + B * w, B + 1)]
    for t, want in sorted(set(edges)):         # (B = 1: origin + width is origin + B * width)
        CASES.append(Case("B=%d t=%d" % (B, t), _ts(str(t)), o, w, B, want))
    CASES.append(Case("B=%d no member" % B, '{"x":1}', o, w, B, B + 2))
    CASES.append(Case("B=%d a string" % B, '{"ts":"105"}', o, w, B, B + 2))
# ---- the whole int64 span ----
CASES += [
    Case("origin INT64_MIN, t INT64_MAX, width 1", _ts(str(I64_MAX)), I64_MIN, 1, 1024, 1025),                 # d = 2^64 - 1
    Case("origin INT64_MIN, t INT64_MAX, width 2^64 - 1", _ts(str(I64_MAX)), I64_MIN, U64_MAX, 4, 1),          # q = 1
    Case("origin INT64_MIN, t INT64_MAX - 1, width 2^64 - 1", _ts(str(I64_MAX - 1)), I64_MIN, U64_MAX, 4, 0),
    Case("origin INT64_MIN, t INT64_MAX, width 2^63", _ts(str(I64_MAX)), I64_MIN, 1 << 63, 2, 1),
    Case("origin INT64_MIN, t -1, width 2^63", _ts("-1"), I64_MIN, 1 << 63, 2, 0),
    Case("origin INT64_MIN, t 0, width 2^63", _ts("0"), I64_MIN, 1 << 63, 2, 1),
    Case("origin INT64_MIN, t INT64_MIN", _ts(str(I64_MIN)), I64_MIN, 7, 3, 0),
    Case("origin INT64_MAX, t INT64_MAX", _ts(str(I64_MAX)), I64_MAX, 1, 1, 0),
    Case("origin INT64_MAX, t INT64_MAX - 1", _ts(str(I64_MAX - 1)), I64_MAX, 1, 1, 1),
    Case("origin INT64_MAX, t 0", _ts("0"), I64_MAX, U64_MAX, 1024, 1024),
    Case("origin 0, width 2^63, t INT64_MAX", _ts(str(I64_MAX)), 0, 1 << 63, 1, 0),
    Case("width 1, the last bucket", _ts("1023"), 0, 1, 1024, 1023),
    Case("width 1, above", _ts("1024"), 0, 1, 1024, 1025),
    # overflowed literals clamp
    Case("an overflowed literal is INT64_MAX", _ts("9" * 30), I64_MAX - 5, 2, 3, 2),
    Case("an overflowed negative literal is INT64_MIN", _ts("-" + "9" * 30), I64_MIN, 1, 1, 0),
    Case("an overflowed negative literal below", _ts("-" + "9" * 30), I64_MIN + 1, 1, 1, 1),
    # fractions floor
    Case("-0.5 is -1: below origin 0", _ts("-0.5"), 0, 1, 4, 4),
    Case("-0.5 is -1: the first bucket from -1", _ts("-0.5"), -1, 1, 4, 0),
    Case("a fraction under a bucket edge", _ts("109.999"), 100, 10, 60, 0),
    Case("a fraction at a bucket edge", _ts("110.000"), 100, 10, 60, 1),
    Case("a fraction over a bucket edge", _ts("110.001"), 100, 10, 60, 1),
    Case("a fraction under the origin", _ts("99.5"), 100, 10, 60, 60),
    Case("a negative fraction at a negative edge", _ts("-10.5"), -20, 10, 2, 0),
    Case("a negative fraction over a negative edge", _ts("-9.5"), -20, 10, 2, 1),
    # the rows the device hands back, at edges of their own
    Case("an exponent at an edge", _ts("1.1e2"), 100, 10, 60, 1, undecided=True),
    Case("an exponent beyond int64", _ts("1e30"), 0, 1, 4, 5, undecided=True),
    Case("an escaped key that is the field", '{"t\\u0073":105}', 100, 10, 60, 0, undecided=True),
    Case("another field name", '{"ts":1,"a.b":25}', 0, 10, 60, 2, field="a.b"),
]
assert len({c.name for c in CASES}) == len(CASES)
