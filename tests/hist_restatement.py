"""A restatement of the bucket rule of bsg_match_rows_wide_hist (include/bloomgpu.h "Bucketed hit counts") in plain Python over exact
ints, built on the MinMax restatement: the field is a top-level key, the last member with it counts, its value must be a number, and
t = clamp(floor(v)).  t < origin is `below`; else q = (t - origin) // width, bucket q or `above`; no such number is `missing`."""
from tests.minmax_restatement import I64_MAX, I64_MIN, row_contributions  # noqa: F401  (re-exported for the tests)

MAX_BUCKETS = 1024


def slots(n_buckets: int) -> int:
    return n_buckets + 3


def below(n_buckets: int) -> int:
    return n_buckets


def above(n_buckets: int) -> int:
    return n_buckets + 1


def missing(n_buckets: int) -> int:
    return n_buckets + 2


def slot_of_value(t, origin: int, width: int, n_buckets: int) -> int:
    """t: the row's value (an int in int64) or None"""
    assert 1 <= n_buckets <= MAX_BUCKETS and 1 <= width < 1 << 64 and I64_MIN <= origin <= I64_MAX
    if t is None:
        return missing(n_buckets)
    if t < origin:
        return below(n_buckets)
    q = (t - origin) // width                  # Python ints: exact, whatever the magnitudes
    return q if q < n_buckets else above(n_buckets)


def slot_of(row: bytes, field: str, origin: int, width: int, n_buckets: int) -> int:
    """The slot of one row.  ValueError when the row is not a JSON object."""
    c = row_contributions(row, [field])
    return slot_of_value(c[field][0] if field in c else None, origin, width, n_buckets)
