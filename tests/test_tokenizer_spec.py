"""Tokenizers of the separator family on the host mirror (bsh_tokenize_with, bsh_entry_sets_index_row_with, the engine
JSON's "Tokenizer") against the Python restatement in tests/tokenizer_restatement.py.  CPU only."""
import ctypes as C
import random

import numpy as np
import pytest

from bloomsearch_amd import _lib, host as Hst
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from tests import tokenizer_restatement as R
from tests.test_host_tables import JSON_MATCHING, _random_value, go_marshal

# what a corpus string is made of: words, separators, case pairs that lower across the ASCII line (U+212A KELVIN SIGN -> k,
# U+0130 -> i), Unicode white space (U+00A0, U+3000), other scripts, and invalid UTF-8
PIECES = ["alice", "Bob", "user=alice", "GET /api/v1/users", "error:timeout", "-1.5E-3", "a,b;c", "KIKI", "kiki", "K",
          "İ", " ", "　", " ", "héllo", "ÉTÉ", "Ωmega", "Да", "日本",
          " ", "\t", "\n", ",", ";", ":", "=", "/", ".", "-", "\"", "[", "]", "(", ")", "A", "Z", "z", "\x01", "\x7f",
          b"\xff", b"\xc3", b"\xed\xa0\x80", b"\xe2\x82", b"\xf0\x9f\x98\x80", b"\xc3\xa9"]

CORPUS_SPECS = dict(R.SPECS, **{
    "kelvin_k": Tokenizer("k", lower=True),                       # U+212A lowers to a separator
    "dotted_i": Tokenizer("i ", lower=True),                      # U+0130 too
    "upper_sep_lower": Tokenizer("AZ,", lower=True),              # an upper-case separator never occurs once lowered
    "upper_sep_raw": Tokenizer("AZ,", lower=False),
    "space_no_unicode": Tokenizer(" ", unicode_space=False, lower=True),
    "space_unicode_raw": Tokenizer(" ", unicode_space=True, lower=False),
    "nothing": Tokenizer(""),
    "default": Tokenizer.default(),
})


def corpus(seed, n):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        parts = [rng.choice(PIECES) for _ in range(rng.randint(0, 8))]
        out.append(b"".join(p if isinstance(p, bytes) else p.encode("utf-8") for p in parts))
    return out


def test_tokenize_with_matches_the_restatement():
    texts = corpus(7, 5000)
    n = 0
    for name, spec in CORPUS_SPECS.items():
        for t in texts:
            assert Hst.tokenize(t, spec, as_bytes=True) == R.tokens(t, spec), (name, t)
            n += 1
    assert n >= 5000 * len(CORPUS_SPECS)


def test_named_cases():
    punct = R.SPECS["punct_lower"]
    assert Hst.tokenize("user=alice", punct) == ["user", "alice"]
    assert Hst.tokenize("GET /api/v1/users", punct) == ["get", "api", "v1", "users"]
    assert Hst.tokenize("error:timeout", punct) == ["error", "timeout"]
    assert Hst.tokenize("-1.5e-3", punct) == ["1", "5e", "3"]
    assert Hst.tokenize("-1.5E-3", R.SPECS["punct_raw"]) == ["1", "5E", "3"]
    assert Hst.tokenize("xKy", Tokenizer("k", lower=True)) == ["x", "y"]
    assert Hst.tokenize("xKy", Tokenizer("k", lower=False)) == ["xKy"]
    assert Hst.tokenize("AİB", Tokenizer("i", lower=True)) == ["a", "b"]
    assert Hst.tokenize("aAb", Tokenizer("A", lower=True)) == ["aab"]
    assert Hst.tokenize("a b", Tokenizer(" ", unicode_space=True)) == ["a", "b"]
    assert Hst.tokenize("a b", Tokenizer(" ", unicode_space=False)) == ["a b"]
    assert Hst.tokenize(b"a\xffb", Tokenizer(",", lower=False), as_bytes=True) == [b"a\xffb"]
    assert Hst.tokenize(b"a\xffB", Tokenizer(",", lower=True), as_bytes=True) == [b"a\xef\xbf\xbdb"]


def test_default_spec_equals_bsh_tokenize():
    for t in corpus(11, 3000):
        assert Hst.tokenize(t, Tokenizer.default()) == Hst.tokenize(t)
    d = _lib.Tokenizer()
    assert Hst.lib().bsg_tokenizer_default(C.byref(d)) == 0
    assert (d.sep_ascii[0], d.sep_ascii[1], d.flags, d.reserved) == (*Tokenizer.default().sep_ascii(), 3, 0)
    assert Hst.tokenize("Hello  World　x", d) == ["hello", "world", "x"]


def _rows():
    rows = [r.encode() if isinstance(r, str) else r for r, _ in JSON_MATCHING]
    rng = np.random.default_rng(5)
    for _ in range(400):
        rows.append(go_marshal({"msg": _random_value(rng, 0), "user": _random_value(rng, 1), "a.b": _random_value(rng, 2)}))
    rows += [b'{"msg":"user=alice GET /api/v1/Users"}', b'{"n":-1.5e-3,"t":true,"f":false,"z":null}',
             b'{"e":"a\\u003db\\/c\\"d\\u0001e\\tf"}', b'{"k":"\\u212aELVIN \\u0130x\\u00a0y\\u3000z"}', b'{"s":"\\ud800lone"}']
    return rows


@pytest.mark.parametrize("name", sorted(R.SPECS) + ["default"])
def test_entry_sets_with_spec_match_the_restatement(name):
    spec = R.SPECS.get(name, Tokenizer.default())
    for row in _rows():
        es = Hst.EntrySets()
        es.index_row(row, spec)
        assert es.as_python_sets() == R.entry_sets([row], spec), (name, row)


def test_invalid_specs_are_refused():
    L = Hst.lib()
    p, n = C.c_void_p(), C.c_uint64()
    for sep0, flags, reserved in ((1, 3, 0), (1 << 32, 3, 1), (1 << 32, 4, 0), (1 << 32, 0x80000000, 0)):
        t = _lib.Tokenizer()
        t.sep_ascii[0], t.flags, t.reserved = sep0, flags, reserved
        assert L.bsh_tokenize_with(b"a b", 3, C.byref(t), C.byref(p), C.byref(n)) == -1      # BSH_E_INVALID
        es = Hst.EntrySets()
        with pytest.raises(Hst.HostError):
            es.index_row(b'{"a":"b"}', t)
    for bad in ("é", "\0", "a　"):
        with pytest.raises(ValueError):
            Tokenizer(bad)
    # the engine JSON: a NUL or non-ASCII separator, or a Tokenizer that is not an object, is ErrInvalidConfig.  bse_open checks
    # the config before the context, so no device is needed: a valid config without a context is BSH_E_INVALID
    for cfg in ('{"Tokenizer":{"Separators":"é"}}', '{"Tokenizer":{"Separators":"\\u0000"}}', '{"Tokenizer":"x"}',
                '{"Tokenizer":{"Separators":5}}'):
        b = cfg.encode()
        h = C.c_void_p()
        assert L.bse_open(b, len(b), None, C.byref(h)) == -101, cfg
        assert not h.value
    for cfg in ('{"Tokenizer":{"Separators":",;","Lower":true}}', '{"Tokenizer":{}}', "{}"):
        b = cfg.encode()
        h = C.c_void_p()
        assert L.bse_open(b, len(b), None, C.byref(h)) == -1, cfg
        assert not h.value
    t = _lib.Tokenizer()
    t.sep_ascii[0], t.flags = 1 << 32, 4
    with pytest.raises(Hst.HostError):
        Hst.match_row(None, b'{"a":"b"}', t)


@pytest.mark.parametrize("name", sorted(R.SPECS) + ["default"])
def test_host_row_matcher_with_spec_matches_the_restatement(name):
    """bsh_match_row_with: the host matcher the rows bsg_match_rows_tok hands back are decided by."""
    from tests.test_tokenizer_match_gpu import expr, rows_for
    spec = R.SPECS.get(name, Tokenizer.default())
    r = random.Random("host-" + name)
    rows = rows_for(6)[:300]
    for _ in range(30):
        bloom = expr(r)
        for row in rows:
            assert Hst.match_row(bloom, row, spec) == R.row_verdict(row, spec, bloom), (name, bloom, row)
