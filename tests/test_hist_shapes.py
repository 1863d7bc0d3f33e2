"""The bucket rule on the host: every case of tests/hist_shapes.py against the restatement (tests/hist_restatement.py) and against
bsh_hist_row (host/minmax.hpp hist_row_slot), the exponent and escaped-key rows included — the host decides every row."""
import pytest

from bloomsearch_amd import host
from tests import hist_restatement as HR
from tests import hist_shapes as HS
from tests import minmax_shapes as MS


@pytest.mark.parametrize("case", HS.CASES, ids=lambda c: c.name)
def test_a_case_lands_in_the_slot_it_names(case):
    want = HR.slot_of(case.row, *case.spec)
    if case.want is not None:
        assert want == case.want
    assert 0 <= want < HR.slots(case.n_buckets)
    assert host.hist_row(case.row, *case.spec) == want


def test_the_cases_cover_the_contract():
    B = lambda c: c.n_buckets
    kinds = {"below": 0, "first": 0, "last": 0, "above": 0, "missing": 0}
    for c in HS.CASES:
        s = HR.slot_of(c.row, *c.spec)
        kinds["below"] += s == B(c)
        kinds["first"] += s == 0
        kinds["last"] += s == B(c) - 1
        kinds["above"] += s == B(c) + 1
        kinds["missing"] += s == B(c) + 2
    assert all(v >= 3 for v in kinds.values()), kinds
    assert {1, 60, 1024} <= {B(c) for c in HS.CASES}
    assert {1, 1 << 63, (1 << 64) - 1} <= {c.width for c in HS.CASES}
    assert {HR.I64_MIN, HR.I64_MAX} <= {c.origin for c in HS.CASES}
    assert sum(c.undecided for c in HS.CASES) >= len(MS.UNDECIDED) + 3
    assert all(b"e" in c.row.lower() or b"\\" in c.row for c in HS.CASES if c.undecided)


def test_the_synthetic_rows_spread_over_the_slots():
    got = {HR.slot_of(HS.synth_row(i), "ts", -40000, 1400, 60) for i in range(3000)}
    assert got == set(range(62))               # every bucket, below and above; every synthetic row has the member


def test_rows_that_are_no_objects_and_bad_arguments_are_refused():
    for row in MS.MALFORMED:
        with pytest.raises(host.HostError):
            host.hist_row(row, "ts", 0, 1, 4)
        with pytest.raises(ValueError):
            HR.slot_of(row, "ts", 0, 1, 4)
    for field, width, n in [("", 1, 4), ("y" * 65, 1, 4), ("ts", 0, 4), ("ts", 1, 0), ("ts", 1, 1025)]:
        with pytest.raises(host.HostError):
            host.hist_row(b'{"ts":1}', field, 0, width, n)
    assert host.hist_row(b'{"%s":7}' % (b"y" * 64), "y" * 64, 0, 1, 1024) == 7
