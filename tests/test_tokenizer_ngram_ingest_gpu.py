"""Device ingest under a spec with an n-gram width (k_ingest_rows_gram, k_ingest_rows_sets_gram) against the Python restatement
(tests/ngram_restatement.py): the three distinct sets' exact counts, and bitsets bit-identical to the oracle's build of the
restated entry sets, for every set and the file-level parent — through the one-shot call (validated and trusted), a stream of
three appends with the rows of two sets interleaved, and two devices with 64 KiB upload chunks.  Rows the device hands back
are walked by the host mirror under the same spec."""
import functools

import numpy as np
import pytest

from bloomsearch_amd import _lib, ingest as I
from bloomsearch_amd._lib import BloomGpuError
from bloomsearch_amd.gpu import Context
from bloomsearch_amd.tokenizer import Tokenizer
from tests import ngram_restatement as G
from tests.helpers import device_ids
from tests.test_host_tables import _random_value, go_marshal
from tests.test_tokenizer_ingest_gpu import EDGE_ROWS, FALLBACK_ROWS, FPR, TRUSTED, check

pytestmark = pytest.mark.gpu

WORD40 = "abcdefghijklmnopqrstuvwxyz0123456789ABCD"       # 40 runes: its windows begin at every offset of an 8-byte chunk
HAND_ROWS = [r.encode("utf-8") for r in (
    '{"w":"a ab abc abcd abcde abcdef"}',                                             # words of n - 1, n and n + 1 runes for n = 2, 3, 4
    '{"two":"é éé ééé éééé ééééé xéyéz"}',                                            # 2-byte runes
    '{"three":"日 日本 日本語 日本語日 日本語日本 a日b本c"}',                              # 3-byte runes
    '{"four":"😀😁😂😃 x😀😁😂😃y 😀 😀😁 😀😁😂 a😀b😁c😂d😃e"}',                         # 4-byte runes; four in a row: the 16-byte window
    '{"stroke":"ȺȺb Ⱥ ȺbȺȺȺ xȺ"}',                                                    # lowering lengthens the rune (2 -> 3 bytes)
    '{"k":"\\u212aELVIN Kelvin \\u0130stanbul İxK iİ"}',            # U+212A -> k, U+0130 -> i, escaped and raw
    '{"e":"ab\\u003dcd x\\"y\\"z q\\tr\\tst \\u003d\\u003d\\u003d\\u003d"}',           # = " and TAB inside a window
    '{"long":"%s","p":"x%s","pp":"xy%sé","ppp":"é%s"}' % ((WORD40,) * 4),             # ... at every alignment of the row
    '{"n":-1.5e-3,"m":1E5,"o":[0,12.25,-7.125e+10,3],"t":true,"f":false,"z":null}',
    '{"arr":["alpha","be","gamma delta",["x","yz","true"]],"deep":{"a":{"b":"nested words here"}}}',
    '{"one":"x","uni":"é","emo":"😀","cjk":"日"}',                                     # leaves of exactly one rune
    '{"mixed":"Hello ok HÉLLO Ωmega-Да/日本 user=alice GET /api/v1/Users"}',
)]


@functools.lru_cache(maxsize=None)
def row_sets(n_sets=3):
    """a few hundred rows in n_sets sets: EDGE_ROWS + FALLBACK_ROWS, 300 go_marshal rows, the hand-written rows"""
    rng = np.random.default_rng(41)
    sets = [[] for _ in range(n_sets)]
    for i in range(300):
        sets[i % n_sets].append(go_marshal({"msg": _random_value(rng, 0), "user": _random_value(rng, 1), "a.b": _random_value(rng, 2)}))
    for i, r in enumerate(EDGE_ROWS + HAND_ROWS):
        sets[i % n_sets].append(r)
        sets[(i + 1) % n_sets].append(r)
    for i, r in enumerate(FALLBACK_ROWS):
        sets[i % n_sets].insert(7 * i, r)
    return tuple(tuple(s) for s in sets)


@functools.lru_cache(maxsize=None)
def want_sets(name, n_sets=3):
    """the restatement's entry sets of every set, then of their union (the parent): computed once per spec"""
    per_set = [G.entry_sets(rows, G.SPECS[name]) for rows in row_sets(n_sets)]
    union = (set(), set(), set())
    for sets in per_set:
        for u, x in zip(union, sets):
            u |= x
    return per_set + [union]


def check_all(res, name, n_sets=3):
    want = want_sets(name, n_sets)
    assert not np.asarray(res.status).any()
    for s in range(n_sets):
        check(res, s, want[s], "%s set %d" % (name, s))
    check(res, n_sets, want[n_sets], name + " parent")


def fallback_index(rs):
    flat = [r for rows in rs for r in rows]
    return {i for i, r in enumerate(flat) if r in FALLBACK_ROWS}


def test_the_rows_cover_the_window_edges():
    """what the hand-written rows are there for, stated on the restatement"""
    spec = G.SPECS["four_nosep_raw"]
    toks = {t for r in HAND_ROWS for t in G.row_tokens(r, spec)}
    assert max(len(t) for t in toks) == 16 and "😀😁😂😃".encode() in toks
    tri = {t for r in HAND_ROWS for t in G.row_tokens(r, G.SPECS["tri_default"])}
    assert {b"a", b"ab", b"abc", b"bcd", "ⱥⱥb".encode(), b"kel", b"ist", b"tru", b"rue", b"als", b"-1.", b"e-3", b"x"} <= tri
    assert {WORD40[i:i + 3].lower().encode() for i in range(38)} <= tri
    assert {b'x"y', b'"y"', b"b=c"} <= tri and b"q\tr\t" in toks


@pytest.mark.parametrize("flags", [0, TRUSTED], ids=["validated", "trusted"])
@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_one_shot_ingest_matches_the_restatement(ctx, name, flags):
    rs = [list(s) for s in row_sets()]
    res = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, flags=flags, tokenizer=G.SPECS[name])
    assert [int(i) for i in res.fallback_rows] == sorted(fallback_index(rs))    # exactly FALLBACK_ROWS are handed back (and walked by the host
    assert len(res.fallback_rows) == len(FALLBACK_ROWS)                        # mirror): the device walks every other row
    check_all(res, name)


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_stream_of_three_appends_matches_the_restatement(ctx, name):
    """two sets whose rows alternate inside every append; the third set arrives whole in the last one"""
    spec = G.SPECS[name]
    rs = row_sets()
    a, b, c = rs
    inter, sor = [], []
    for i in range(max(len(a), len(b))):
        for s, rows in ((0, a), (1, b)):
            if i < len(rows):
                inter.append(rows[i])
                sor.append(s)
    cut1, cut2 = len(inter) // 3 + 1, 2 * len(inter) // 3
    with I.IngestStream.open(ctx, 3, [0, 0, 0], 1, tokenizer=spec) as st:
        handed = 0
        handed += len(st.append(inter[:cut1], sor[:cut1]))
        handed += len(st.append(inter[cut1:cut2], sor[cut1:cut2]))
        handed += len(st.append(inter[cut2:] + list(c), sor[cut2:] + [2] * len(c)))
        assert handed == len(FALLBACK_ROWS)
        counts, status = st.finish()
        desc, n_words = I.plan_desc(counts, FPR)
        words = st.build(desc, n_words)
    check_all(I.IngestResult(counts, status, desc, words, None, None), name)


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_two_devices_in_64_kib_chunks(name):
    with Context(device_ids(2)) as m:
        m.set_lab(8, 1)                                     # shard whatever the size
        m.set_ingest_chunk(1 << 16)
        rs = [list(s) for s in row_sets(4)]
        res = I.device_ingest(m, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, tokenizer=G.SPECS[name])
        check_all(res, name, 4)


def test_width_0_ingests_what_the_spec_without_the_field_ingests(ctx):
    from tests import tokenizer_restatement as R
    rs = [list(s) for s in row_sets()]
    spec = R.SPECS["punct_lower"]
    t = spec.to_c()
    t.flags |= _lib.TOK_NGRAM(0)
    a = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, tokenizer=spec)
    b = I.device_ingest(ctx, rs, FPR, parent_of_set=[0] * len(rs), n_parents=1, tokenizer=t)
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.desc, b.desc) and np.array_equal(a.words, b.words)
    assert np.array_equal(a.fallback_rows, b.fallback_rows)


def test_the_device_refuses_other_widths(ctx):
    rows = [b'{"msg":"abcdef"}']
    for width in (1, 5, 6, 7):
        t = Tokenizer.default().to_c()
        t.flags |= width << _lib.TOK_NGRAM_SHIFT
        with pytest.raises(BloomGpuError) as e:
            ctx.ingest_rows(rows, np.array([0, 1], dtype=np.uint32), tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID and "width %d" % width in str(e.value)
        with pytest.raises(BloomGpuError) as e:
            ctx.ingest_open(1, [0], 1, tokenizer=t)
        assert e.value.code == _lib.BSG_E_INVALID
    res = I.device_ingest(ctx, [rows], FPR, tokenizer=G.SPECS["tri_default"])
    assert [int(x) for x in res.counts[0]] == [1, 4, 4] and len(res.fallback_rows) == 0      # abc bcd cde def
