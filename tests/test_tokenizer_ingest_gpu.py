"""bsg_ingest_rows_tok (k_ingest_rows under a separator-family tokenizer spec) against the Python restatement
(tests/tokenizer_restatement.py): exact distinct counts, and bitsets bit-identical to the oracle's build of the restated
entry sets, for the blocks and their file-level parent; rows the device hands back are finished by the host walker with
the same spec."""
import numpy as np
import pytest

from bloomsearch_amd import ingest as I, synth
from bloomsearch_amd.gpu import Context
from oracle import oracle as O
from tests import tokenizer_restatement as R
from tests.helpers import device_ids
from tests.test_host_tables import _random_value, go_marshal

pytestmark = pytest.mark.gpu

FPR = 0.001
TRUSTED = 1   # BSG_INGEST_TRUSTED_JSON

EDGE_ROWS = [
    b'{"msg":"user=alice GET /api/v1/Users error:timeout"}',
    b'{"e":"a\\u003db\\/c\\"d\\\\e\\tf(g)[h]"}',                   # escapes that decode to separators
    b'{"n":-1.5e-3,"m":1E5,"o":[0,12.25,-7],"t":true,"f":false,"z":null}',
    b'{"u":"\\u212aELVIN \\u0130stanbul x\\u00a0y\\u3000z \xe2\x84\xaa \xc4\xb0"}',
    b'{"w":"a,b;c:d=e/f.g-h \\"quoted\\" (paren) [br]","K":"KEY=Value"}',
    b'{"deep":{"a":{"b":{"c":"x.y-z"}}},"arr":[{"k":"v=w"},"p;q"]}',
    b'{"ctl":"a\\u0002b\\u001fc"}',
]
FALLBACK_ROWS = [
    b'{"s":"\\ud800lone=surrogate"}',                                # a lone surrogate escape: the host walker's
    b'{"d":"del\x7fbyte=x"}',                                        # a raw DEL: the host walker's
    b'{"' + b'k' * 120 + b'":"long=path"}',                          # a path longer than the device keeps
    b'{"a":' * 20 + b'"deep=value"' + b'}' * 20,                     # nested deeper than the device walks
]


def row_sets(seed, n_sets=3, per_set=300, with_fallback=True):
    rng = np.random.default_rng(seed)
    sets = []
    for s in range(n_sets):
        rows = list(synth.rows_json(s * per_set, per_set // 2))
        for _ in range(per_set // 2):
            rows.append(go_marshal({"msg": _random_value(rng, 0), "user": _random_value(rng, 1), "a.b": _random_value(rng, 2)}))
        rows += EDGE_ROWS
        if with_fallback:
            rows += FALLBACK_ROWS[s % len(FALLBACK_ROWS):][:2]
        sets.append(rows)
    return sets


def check(res, set_index, sets, what):
    for kind in range(3):
        assert int(res.counts[set_index, kind]) == len(sets[kind]), (what, kind)
        want = O.build_sized(sorted(sets[kind]), FPR)
        d = res.desc[set_index * 3 + kind]
        assert (int(d["m"]), int(d["k"])) == (want.m, want.k), (what, kind)
        assert np.array_equal(res.filter_words(set_index, kind), want.words), (what, kind)


def check_all(res, rs, spec):
    union = (set(), set(), set())
    for s, rows in enumerate(rs):
        sets = R.entry_sets(rows, spec)
        check(res, s, sets, "set %d" % s)
        for u, x in zip(union, sets):
            u |= x
    check(res, len(rs), union, "parent")


@pytest.mark.parametrize("flags", [0, TRUSTED], ids=["validated", "trusted"])
@pytest.mark.parametrize("name", sorted(R.SPECS))
def test_ingest_rows_tok_matches_the_restatement(ctx, name, flags):
    spec = R.SPECS[name]
    rs = row_sets(3)
    res = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, flags=flags, tokenizer=spec)
    flat = [r for rows in rs for r in rows]                          # exactly FALLBACK_ROWS are handed back (and finished by the host walker):
    assert [int(i) for i in res.fallback_rows] == [i for i, r in enumerate(flat) if r in FALLBACK_ROWS]      # no other row leaves the device
    assert len(res.fallback_rows) == 2 * len(rs)
    check_all(res, rs, spec)


def test_punctuation_spec_finds_words_the_default_cannot(ctx):
    rows = [[b'{"msg":"user=alice"}']]
    punct = I.device_ingest(ctx, rows, FPR, tokenizer=R.SPECS["punct_lower"])
    plain = I.device_ingest(ctx, rows, FPR)
    assert [int(x) for x in punct.counts[0]] == [1, 2, 2] and [int(x) for x in plain.counts[0]] == [1, 1, 1]
    check(punct, 0, R.entry_sets(rows[0], R.SPECS["punct_lower"]), "punct")


def test_default_plus_0x01_is_bit_identical_to_the_default(ctx):
    """Default separators plus byte 0x01 forces the TokSpec kernel; on rows that never decode to 0x01 it emits what
    k_ingest_rows emits."""
    rs = row_sets(9, with_fallback=True)
    rs = [[r for r in rows if b"\\u0001" not in r] for rows in rs]
    for flags in (0, TRUSTED):
        a = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, flags=flags, tokenizer=R.SPECS["default_plus_01"])
        b = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, flags=flags)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.status, b.status)
        assert np.array_equal(a.desc, b.desc) and np.array_equal(a.words, b.words)
        assert np.array_equal(a.fallback_rows, b.fallback_rows)


def test_ingest_rows_tok_on_two_devices():
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        spec = R.SPECS["punct_lower"]
        rs = row_sets(4, n_sets=4)
        res = I.device_ingest(m, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, tokenizer=spec)
        check_all(res, rs, spec)
