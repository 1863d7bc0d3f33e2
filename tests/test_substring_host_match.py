"""bsh_match_row_substring, the exact substring test on the host (the matcher of fallback rows and the oracle of the device tests),
against a Python restatement: leaf texts from oracle/walker_oracle.py, folded with its one-rune lower table, compared with `in`
(tests/substring_restatement.py)."""
import json

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from tests import substring_restatement as SR
from tests.test_host_tables import KEYS, _random_value, go_marshal

ROW = b'{"a":{"b":"Hello W\\u00e9rld\\nNext","c":null,"n":1E5,"t":true},"needle":"hay","arr":["con","nect"],"a.x":"dotted"}'
SPECS = {"default": None, "trigram": SR.TRIGRAM, "punct": SR.PUNCT, "raw": SR.RAW}


def both(sub, row, tok=None):
    got = Hst.match_row_substring(sub, row, tok)
    assert got == SR.row_verdict(row, sub, tok), (sub, row)
    return got


@pytest.mark.parametrize("spec", sorted(SPECS))
def test_fixed_cases(spec):
    tok = SPECS[spec]
    lower = spec != "raw"
    assert not both(Q.Substring("needle"), ROW, tok)                                  # only in a key
    assert not both(Q.Substring("null"), ROW, tok)                                    # only in null
    assert both(Q.Substring("E5"), ROW, tok)                                          # a number's raw literal
    assert both(Q.Substring("e5"), ROW, tok) == lower
    assert both(Q.Substring("ru"), ROW, tok)                                          # true
    assert both(Q.Substring("Wérld\nN"), ROW, tok)                               # across the é and \n escapes
    assert both(Q.Substring("wÉRLD\nn"), ROW, tok) == lower
    assert not both(Q.Substring("connect"), ROW, tok)                                 # split over two leaves
    assert both(Q.Substring("nect"), ROW, tok)
    assert not both(Q.FieldSubstring("a", "Hello"), ROW, tok)                         # a does not see the leaf a.b
    assert both(Q.FieldSubstring("a.b", "Hello"), ROW, tok)
    assert both(Q.FieldSubstring("arr", "on"), ROW, tok)                              # array elements have the array's path
    assert both(Q.FieldSubstring("a.x", "dot"), ROW, tok)
    assert not both(Q.FieldSubstring("a.c", "null"), ROW, tok)
    assert not both(Q.FieldSubstring("", "hay"), ROW, tok)
    assert both(Q.SubstringAnd(Q.Substring("hay"), Q.SubstringOr(Q.Substring("zzz"), Q.FieldSubstring("a.t", "true"))), ROW, tok)
    assert not both(Q.SubstringOr(), ROW, tok) and both(Q.SubstringAnd(), ROW, tok)
    assert both({"ExpressionType": "CONDITION", "Condition": None}, ROW, tok) and both(None, ROW, tok)
    assert not both({"ExpressionType": "XOR", "Children": []}, ROW, tok)


def test_the_kelvin_sign_folds_to_k_and_root_scalars_are_no_leaves():
    assert both(Q.Substring("akb"), '{"t":"aKb"}'.encode()) and both(Q.Substring("aKb"), b'{"t":"AKB"}')
    assert not both(Q.Substring("aKb"), b'{"t":"AKB"}', SR.RAW)
    assert not both(Q.Substring("x"), b'"x"') and not both(Q.Substring("x"), b'{"":"x"}')


def test_random_rows_and_needles_cut_from_their_texts():
    rng = np.random.default_rng(21)
    n = 0
    for i in range(400):
        row = go_marshal({KEYS[rng.integers(0, len(KEYS))]: _random_value(rng, 0) for _ in range(rng.integers(1, 6))})
        for spec in (None, SR.RAW, SR.TRIGRAM):
            texts = [(p, SR.fold(t, SR.spec_of(spec))) for p, leaf, t in SR.TR.leaves(row) if leaf and t]
            if not texts:
                continue
            p, t = texts[rng.integers(0, len(texts))]
            rs = SR.runes(t)
            a = int(rng.integers(0, len(rs)))
            b = min(len(rs), a + int(rng.integers(1, 12)))
            needle = b"".join(rs[a:b])
            if len(needle) > 64 or b"\xef\xbf\xbd" in needle:
                continue
            nd = needle.decode("utf-8")
            assert both(Q.Substring(nd), row, spec) and both(Q.FieldSubstring(p, nd), row, spec)
            both(Q.FieldSubstring(p + "x", nd), row, spec)
            both(Q.Substring(nd + "éq"), row, spec)
            n += 1
    assert n > 600


def test_needle_limits():
    for bad, code in (("", -1), ("x" * 65, -5)):
        with pytest.raises(Hst.HostError) as ei:
            Hst.match_row_substring(Q.Substring(bad), ROW)
        assert ei.value.code == code
    L = Hst.lib()
    s = b'{"ExpressionType":"CONDITION","Condition":{"Needle":"a\xffb"}}'
    assert L.bsh_match_row_substring(s, len(s), ROW, len(ROW), None) == -1            # invalid UTF-8 (the JSON reader lets the byte through)
    assert Hst.match_row_substring(Q.Substring("x" * 64), ROW) is False
