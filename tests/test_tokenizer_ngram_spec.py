"""N-gram tokens of a separator-family spec (bloomgpu.h BSG_TOK_NGRAM) on the host mirror — bsh_tokenize_with,
bsh_entry_sets_index_row_with, bsh_match_row_with, the engine JSON's "Tokenizer": {"Ngram": n} — against the Python restatement
in tests/ngram_restatement.py.  CPU only."""
import ctypes as C
import random

import pytest

from bloomsearch_amd import _lib, host as Hst
from bloomsearch_amd.tokenizer import Tokenizer
from tests import ngram_restatement as G, tokenizer_restatement as R
from tests.test_tokenizer_spec import _rows, corpus

DEFAULT = Tokenizer.default()


def gram(spec: Tokenizer, n: int) -> Tokenizer:
    return Tokenizer(spec.separators, unicode_space=spec.unicode_space, lower=spec.lower, ngram=n)


FOUR_FACES = "x\U0001F600\U0001F601\U0001F602\U0001F603y"
# the issue's table: (spec, text, n, tokens)
WORKED = [
    (DEFAULT, "Hello ok", 3, ["hel", "ell", "llo", "ok"]),
    (DEFAULT, "héllo", 2, ["hé", "él", "ll", "lo"]),
    (DEFAULT, "abc abcd abcde", 4, ["abc", "abcd", "abcd", "bcde"]),
    (Tokenizer(""), "ab cd", 3, ["ab ", "b c", " cd"]),
    (DEFAULT, "KELVIN", 3, ["kel", "elv", "lvi", "vin"]),
    (DEFAULT, "-1.5e-3", 3, ["-1.", "1.5", ".5e", "5e-", "e-3"]),
    (DEFAULT, "true", 3, ["tru", "rue"]),
    (DEFAULT, "ȺȺb", 2, ["ⱥⱥ", "ⱥb"]),
    (Tokenizer(""), FOUR_FACES, 4, ["x\U0001F600\U0001F601\U0001F602", "\U0001F600\U0001F601\U0001F602\U0001F603",
                                    "\U0001F601\U0001F602\U0001F603y"]),
]


@pytest.mark.parametrize("case", range(len(WORKED)))
def test_worked_values(case):
    spec, text, n, want = WORKED[case]
    spec = gram(spec, n)
    assert [t.decode() for t in G.tokens(text, spec)] == want            # the restatement states the definition
    assert Hst.tokenize(text, spec) == want
    assert all(len(t.encode()) <= 16 for t in want)


def test_the_largest_window_is_16_bytes_and_lowering_lengthens_runes():
    got = Hst.tokenize(FOUR_FACES, Tokenizer("", ngram=4), as_bytes=True)
    assert [len(t) for t in got] == [13, 16, 13]
    got = Hst.tokenize("ȺȺb", gram(DEFAULT, 2), as_bytes=True)
    assert [len(t) for t in got] == [6, 4] and len("ȺȺb".encode()) == 5


def test_invalid_bytes_are_runes_of_width_one():
    raw = Tokenizer(",", lower=False, ngram=2)
    low = Tokenizer(",", lower=True, ngram=2)
    assert Hst.tokenize(b"a\xffb", raw, as_bytes=True) == [b"a\xff", b"\xffb"] == G.tokens(b"a\xffb", raw)
    assert Hst.tokenize(b"a\xffB", low, as_bytes=True) == [b"a\xef\xbf\xbd", b"\xef\xbf\xbdb"] == G.tokens(b"a\xffB", low)
    assert Hst.tokenize(b"\xe2\x82,\xf0\x9f", raw, as_bytes=True) == [b"\xe2\x82", b"\xf0\x9f"]      # two runes each: the words whole


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_tokenize_with_matches_the_restatement(name):
    spec = G.SPECS[name]
    texts = corpus(23, 3000)
    windows = 0
    for t in texts:
        want = G.tokens(t, spec)
        assert Hst.tokenize(t, spec, as_bytes=True) == want, (name, t)
        windows += len(want) - len(R.tokens(t, spec))
    assert windows > 3000                                                # the corpus does cut words into windows


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_entry_sets_match_the_restatement(name):
    spec = G.SPECS[name]
    for row in _rows():
        es = Hst.EntrySets()
        es.index_row(row, spec)
        assert es.as_python_sets() == G.entry_sets([row], spec), (name, row)


@pytest.mark.parametrize("name", sorted(R.SPECS) + ["default"])
def test_width_0_is_the_spec_without_the_field(name):
    spec = R.SPECS.get(name, DEFAULT)
    zero = gram(spec, 0)
    assert zero.to_c().flags == spec.to_c().flags and zero.to_json() == spec.to_json()
    t = spec.to_c()
    t.flags |= _lib.TOK_NGRAM(0)
    for text in corpus(29, 1500):
        want = Hst.tokenize(text, spec, as_bytes=True)
        assert Hst.tokenize(text, zero, as_bytes=True) == want and Hst.tokenize(text, t, as_bytes=True) == want
        assert G.tokens(text, zero) == want


def test_widths_1_5_6_7_are_refused():
    L = Hst.lib()
    p, n = C.c_void_p(), C.c_uint64()
    for width in (1, 5, 6, 7):
        t = DEFAULT.to_c()
        t.flags |= width << _lib.TOK_NGRAM_SHIFT
        assert t.flags & ~_lib.TOK_NGRAM_MASK == 3
        assert L.bsh_tokenize_with(b"a b", 3, C.byref(t), C.byref(p), C.byref(n)) == -1      # BSH_E_INVALID
        with pytest.raises(Hst.HostError):
            Hst.EntrySets().index_row(b'{"a":"b"}', t)
        with pytest.raises(Hst.HostError):
            Hst.match_row(None, b'{"a":"b"}', t)
        with pytest.raises(ValueError):
            Tokenizer(" ", ngram=width)
        b = ('{"Tokenizer":{"Separators":" ","Ngram":%d}}' % width).encode()
        h = C.c_void_p()
        assert L.bse_open(b, len(b), None, C.byref(h)) == -101, b                          # ErrInvalidConfig
        assert not h.value
    for width in (2, 3, 4):
        t = DEFAULT.to_c()
        t.flags |= _lib.TOK_NGRAM(width)
        assert L.bsh_tokenize_with(b"a b", 3, C.byref(t), C.byref(p), C.byref(n)) == 0
        L.bsh_free(p)
    for bad in (True, 2.0, "3", -2, 8):
        with pytest.raises(ValueError):
            Tokenizer(" ", ngram=bad)


def test_ngram_in_the_engine_config():
    """bse_open checks the config before the context: a valid config without a context is BSH_E_INVALID (-1), an invalid one
    ErrInvalidConfig (-101)."""
    L = Hst.lib()
    for cfg, want in (('{"Tokenizer":{"Separators":" ","Lower":true,"Ngram":3}}', -1), ('{"Tokenizer":{"Ngram":2}}', -1),
                      ('{"Tokenizer":{"Ngram":4}}', -1), ('{"Tokenizer":{"Ngram":0}}', -1), ('{"Tokenizer":{"Separators":" "}}', -1),
                      ('{"Tokenizer":{"Ngram":2.5}}', -101), ('{"Tokenizer":{"Ngram":3.0}}', -101), ('{"Tokenizer":{"Ngram":"3"}}', -101),
                      ('{"Tokenizer":{"Ngram":true}}', -101), ('{"Tokenizer":{"Ngram":-3}}', -101), ('{"Tokenizer":{"Ngram":8}}', -101),
                      ('{"Tokenizer":{"Ngram":13}}', -101), ('{"Tokenizer":{"Ngram":3e0}}', -101)):
        b = cfg.encode()
        h = C.c_void_p()
        assert L.bse_open(b, len(b), None, C.byref(h)) == want, cfg
        assert not h.value
    assert G.SPECS["tri_default"].to_json()["Ngram"] == 3 and "Ngram" not in DEFAULT.to_json()


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_host_row_matcher_matches_the_restatement(name):
    """bsh_match_row_with: the host matcher that decides the rows the device matchers hand back."""
    from tests.test_tokenizer_ngram_match_gpu import expr, rows_and_pool
    spec = G.SPECS[name]
    rows, pool = rows_and_pool(name)
    r = random.Random("host-" + name)
    rows = rows[:200]
    for _ in range(15):
        bloom = expr(r, pool)
        for row in rows:
            assert Hst.match_row(bloom, row, spec) == G.row_verdict(row, spec, bloom), (name, bloom, row)
