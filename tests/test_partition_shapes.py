"""The keyed ingest's partition rule on the host: the shapes' STATED texts and hand-backs against the restatement, and
bsh_partition_key against both.  bsh_partition_key is validate_object_row (host/partition.hpp calls it and nothing else), the
function the engine has always partitioned by; the engine itself is compared on the device (tests/test_engine_partition_gpu.py)."""
import json

import pytest

from bloomsearch_amd import host as Hst
from tests import partition_restatement as PR
from tests import partition_shapes as PS

IDS = [s.name for s in PS.SHAPES]


@pytest.mark.parametrize("s", PS.SHAPES, ids=IDS)
def test_the_stated_text_is_the_restatements(s):
    json.loads(s.row)                                              # every shape is valid JSON
    assert PR.partition_text(s.row, s.field) == s.text
    assert PR.device_decides(s.row, s.field) == (not s.undecided)


@pytest.mark.parametrize("s", PS.SHAPES, ids=IDS)
def test_bsh_partition_key_gives_the_stated_text(s):
    assert Hst.partition_key(s.row, s.field) == s.text


def test_the_restatement_keeps_the_first_duplicate_and_the_raw_literal():
    assert PR.partition_text(b'{"p":1.0,"p":2}', "p") == b"1.0"
    assert PR.partition_text(b'{"p":-0}', "p") == b"-0" and PR.partition_text(b'{"p":1E5}', "p") == b"1E5"
    assert PR.partition_text(b'{"q":{"p":1}}', "p") == b""
    for bad in (b"[]", b'"p"', b"{", b'{"p":NaN}', b'{"p":1}x'):
        with pytest.raises(ValueError):
            PR.partition_text(bad, "p")
    # numbering: first decided appearance, handed-back rows take none
    sets, keys = PR.assign_sets([[b'{"p":"b"}', b'{"p":"x\\\\"}', b'{"p":"a"}', b'{"p":"b"}'], [b'{}', b'{"p":"a"}']], "p")
    assert sets == [[0, None, 1, 0], [2, 1]] and keys == [b"b", b"a", b""]


def test_bsh_partition_key_refuses_bad_names_and_rows():
    for name in ("", "n" * 65):
        with pytest.raises(Hst.HostError):
            Hst.partition_key(b"{}", name)
    for row in (b"", b"[]", b'{"p":1', b'{"p":1}}', b'{"p":1,}', b'{"p":tru}'):
        with pytest.raises(Hst.HostError):
            Hst.partition_key(row, "p")
    assert Hst.partition_key(b"{}", "n" * 64) == b""


def test_the_alignment_batch_puts_every_shape_at_every_alignment():
    at, seen = 0, {}
    for s, row in PS.at_every_alignment():
        if s is not None:
            seen.setdefault(s.name, set()).add(at % 8)
        at += len(row)
    assert all(seen[s.name] == set(range(8)) for s in PS.SHAPES)
