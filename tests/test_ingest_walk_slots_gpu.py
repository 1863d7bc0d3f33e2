"""The one row walk of the device ingest (ingest_api.inc RowWalk) through each of its six walkers — rows grouped by set (one
bsg_ingest_rows call) or in a staged order (a stream of two appends whose rows alternate between the sets), under the default
tokenizer, a separator spec and a spec with an n-gram width — without and with MinMax fields: twelve walks over the same rows.

The rows: 1 024 of 264 bytes in two sets, uploaded in 64 KiB chunks, so the grouped walk has three chunks (256, 512 and 256 rows) and
each append two; in every chunk of every walk a row nested deeper than the device walker follows, which it hands back; token tables
that start at 64 slots.  The first 128 rows of a set share a few words, every later row brings four of its own: in the grouped walk
set 1 meets its first rows in the second chunk, and the first chunk of the first append leaves every table at 256 slots at the most
(fewer entries than the probe bound: such a table cannot overflow) while its second chunk brings more entries than that — so in both
forms a table must grow in a chunk after the first, behind a handed-back row, and that chunk is walked again.  Asserted against the Python walkers (oracle/walker_oracle.py, tests/tokenizer_restatement.py,
tests/ngram_restatement.py): every table's count is the size of the restated set, the parent's included; the rows handed back are
exactly the planted ones, ascending, each once — also from the chunk that was walked twice; with fields, the index equals
tests/minmax_restatement.py's.  That the restated envelope (tests/walker_envelope_shapes.py) puts exactly the planted rows outside is
checked first and without a device, so no walk can pass by handing every row back."""
import functools
import hashlib

import numpy as np
import pytest

from bloomsearch_amd import ingest as I
from oracle import walker_oracle as W
from tests import minmax_restatement as MR
from tests import ngram_restatement as G
from tests import tokenizer_restatement as R
from tests import walker_envelope_shapes as ENV
from tests.table_shapes import MAX_PROBE
from tests.test_ingest_minmax_gpu import as_lists
from tests.test_row_chunks import ingest_plan_before

FPR = 0.01
N_SETS, PER_SET, ROW_BYTES, CHUNK = 2, 512, 264, 1 << 16
FIELDS = ["ts", "a.b"]
HINT = [0, 64, 64] * N_SETS                     # the token tables start at 64 slots
PLANT_EVERY = 100                               # a planted row at every index that is 7 modulo 100: several in every chunk
FEW_WORDS = 128                                 # the first rows of a set share their words; every later row brings four of its own
TOKENIZERS = {"default": None, "spec": R.SPECS["punct_lower"], "gram": G.SPECS["tri_default"]}


def make_row(s: int, j: int) -> bytes:
    i = s * PER_SET + j
    if j % PLANT_EVERY == 7:                    # 17 containers open at once: outside the walker's envelope, inside the scanner's reach
        head = '{"ts":%d,"a.b":%d,"pad":"' % (5000 + i, -i)
        tail = '","d":' + '{"d":' * 16 + '"deep%d"' % i + "}" * 17
    elif j < FEW_WORDS:
        head = '{"ts":%d,"a.b":%d,"level":"%s","msg":"aa Bb w%d","pad":"' % (1000 + j % 4, j % 3, ("info", "warn", "error")[j % 3], j % 4)
        tail = '"}'
    else:
        own = hashlib.md5(b"%d" % i).hexdigest()
        head = '{"ts":%d,"a.b":%d,"level":"%s","msg":"%s %s %s K%s served","pad":"' % (
            (i * 7919) % 100003 - 50000, i % 11, ("info", "warn", "error")[i % 3], own[:8], own[8:16], own[16:24], own[24:])
        tail = '"}'
    return (head + ("lorem ipsum " * 30)[:ROW_BYTES - len(head) - len(tail)] + tail).encode()


@functools.lru_cache(maxsize=None)
def row_sets():
    return tuple(tuple(make_row(s, j) for j in range(PER_SET)) for s in range(N_SETS))


def planted(rows):
    return [i for i, r in enumerate(rows) if b'"deep' in r]


@functools.lru_cache(maxsize=None)
def batches():
    """two appends, each the next half of every set with the sets alternating row by row -> [(rows, set_of_row)]"""
    out = []
    for lo, hi in ((0, PER_SET // 2), (PER_SET // 2, PER_SET)):
        rows, sets = [], []
        for j in range(lo, hi):
            for s in range(N_SETS):
                rows.append(row_sets()[s][j])
                sets.append(s)
        out.append((rows, sets))
    return out


def entry_sets(tok, rows):
    if tok == "default":
        sets = (set(), set(), set())
        for r in rows:
            W.index_row(r, sets)
        return sets
    return (R if tok == "spec" else G).entry_sets(rows, TOKENIZERS[tok])


@functools.lru_cache(maxsize=None)
def want_sets(tok):
    """the restated entry sets of every set, then of the parent: once per tokenizer"""
    per_set = [entry_sets(tok, rows) for rows in row_sets()]
    return per_set + [tuple(set().union(*(s[k] for s in per_set)) for k in range(3))]


@functools.lru_cache(maxsize=None)
def want_index():
    return MR.set_indexes([list(rs) for rs in row_sets()], FIELDS)


def chunks_of(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return ingest_plan_before(off, len(rows), CHUNK)[0]


def test_the_rows_are_what_the_walks_need():
    """no device: the row size, the chunk plans, a planted row in every chunk, and the restated envelope hands back those alone"""
    flat = [r for rs in row_sets() for r in rs]
    assert all(len(r) == ROW_BYTES for r in flat)
    walks = [flat] + [rows for rows, _ in batches()]
    assert [len(chunks_of(w)) - 1 for w in walks] == [3, 2, 2]
    for w in walks:
        cuts, bad = chunks_of(w), planted(w)
        assert [i for i, r in enumerate(w) if not ENV.in_envelope(r)] == bad          # exactly the planted rows, no others
        assert all(any(a <= i < b for i in bad) for a, b in zip(cuts, cuts[1:]))       # at least one in every chunk
    assert len(planted(flat)) == 12
    # grouped: set 1 meets its first rows in the second chunk, more entries than its 64-slot tables hold: they must grow there, behind
    # the first chunk's handed-back rows
    cuts = chunks_of(flat)
    assert cuts[1] <= PER_SET < cuts[2]
    # by set: the first chunk of the first append leaves every token table at 64 or 256 slots — it brings fewer entries than the probe
    # bound, and a table of 256 with so few cannot send a probe past the bound — and the second chunk brings more than 256: the tables
    # must grow there, behind the first chunk's handed-back rows
    rows_a, sets_a = batches()[0]
    cut_a = chunks_of(rows_a)[1]
    assert planted(rows_a)[0] < cut_a
    for t in TOKENIZERS:
        for s in range(N_SETS):
            second = entry_sets(t, row_sets()[1][:cuts[2] - PER_SET]) if s == 1 else None
            first = entry_sets(t, [r for r, x in zip(rows_a[:cut_a], sets_a[:cut_a]) if x == s])
            both = entry_sets(t, [r for r, x in zip(rows_a, sets_a) if x == s])
            for k in (1, 2):
                assert second is None or len(second[k]) > 64, (t, s, k)
                assert 0 < len(first[k]) < MAX_PROBE and len(both[k]) > 4 * 64, (t, s, k, len(first[k]), len(both[k]))
    # the scanner's fields are plain integers in every row, the planted ones included
    assert all(len(MR.row_contributions(r, FIELDS)) == 2 for r in flat)


def check_counts(counts, status, tok):
    want = want_sets(tok)
    assert not np.asarray(status).any()
    for s in range(N_SETS + 1):
        assert [int(c) for c in counts[s]] == [len(want[s][k]) for k in range(3)], (tok, "parent" if s == N_SETS else "set %d" % s)


@pytest.fixture
def small_chunks(ctx):
    ctx.set_ingest_chunk(CHUNK)
    yield ctx
    ctx.set_ingest_chunk(0)


@pytest.mark.gpu
@pytest.mark.parametrize("minmax", [False, True], ids=["plain", "minmax"])
@pytest.mark.parametrize("tok", sorted(TOKENIZERS))
def test_grouped_rows_through_one_call(small_chunks, tok, minmax):
    rs = [list(s) for s in row_sets()]
    res = I.device_ingest(small_chunks, rs, FPR, parent_of_set=[0] * N_SETS, n_parents=1, slots_hint=HINT, tokenizer=TOKENIZERS[tok],
                          minmax_fields=FIELDS if minmax else None)
    assert res.stats.table_grows >= 1
    assert [int(r) for r in res.fallback_rows] == planted([r for s in rs for r in s])          # ascending, each once
    assert res.stats.n_rows == N_SETS * PER_SET and res.stats.n_fallback_rows == len(res.fallback_rows)
    check_counts(res.counts, res.status, tok)
    if minmax:
        assert as_lists(res.minmax(), len(FIELDS)) == want_index()


@pytest.mark.gpu
@pytest.mark.parametrize("minmax", [False, True], ids=["plain", "minmax"])
@pytest.mark.parametrize("tok", sorted(TOKENIZERS))
def test_rows_by_set_through_two_appends(small_chunks, tok, minmax):
    with I.IngestStream.open(small_chunks, N_SETS, [0] * N_SETS, 1, slots_hint=HINT, tokenizer=TOKENIZERS[tok],
                             minmax_fields=FIELDS if minmax else None) as st:
        for rows, sets in batches():
            fb = st.append(rows, sets)
            assert [int(r) for r in fb] == planted(rows)                                        # ascending, each once
        counts, status = st.finish()
        stats = st.stats()
        assert stats.table_grows >= 1 and stats.n_rows == N_SETS * PER_SET and stats.n_fallback_rows == 12
        check_counts(counts, status, tok)
        if minmax:
            assert as_lists(st.minmax(), len(FIELDS)) == want_index()
