"""substring_terms and the substring guard (host/substring.hpp) through the library: fixed vectors, the no-false-negative property
against the tokenizer (every term of a needle cut from a text is a token of that text), the guard's shape, and bsh_prune_query_sub
against bsh_prune_query.  The Python side folds with the restatements' tables (tests/substring_restatement.py), never str.lower."""
import dataclasses

import numpy as np
import pytest

from bloomsearch_amd import host as Hst, query as Q
from bloomsearch_amd.tokenizer import WHITE_SPACE, Tokenizer
from tests import substring_restatement as SR

TRI = SR.TRIGRAM
WORD = Tokenizer.default()
WINDOWS = lambda w: [w[i:i + 3] for i in range(len(w) - 2)]


def test_fixed_vectors_on_the_trigram_spec():
    assert Hst.substring_terms("timeout", TRI) == ["tim", "ime", "meo", "eou", "out"]
    assert Hst.substring_terms("TimeOut", TRI) == ["tim", "ime", "meo", "eou", "out"]
    assert Hst.substring_terms("on re", TRI) == []                       # two partial words shorter than the width
    assert Hst.substring_terms("by", TRI) == []
    assert Hst.substring_terms(" by ", TRI) == ["by"]                    # a whole short word is a token as itself
    assert Hst.substring_terms("connection reset by peer", TRI) == WINDOWS("connection") + ["res", "ese", "set", "by", "pee", "eer"]
    assert len(WINDOWS("connection")) == 8
    assert Hst.substring_terms("aKb", TRI) == ["akb"]                # U+212A KELVIN SIGN lowers to k
    assert Hst.substring_terms("xaKb", TRI) == ["xak", "akb"]
    assert Hst.substring_terms("Étés", TRI) == ["été", "tés"]      # windows are runes, not bytes


def test_without_a_width_only_whole_words_are_terms():
    for spec in (WORD, None):
        assert Hst.substring_terms("connection reset by peer", spec) == ["reset", "by"]
        assert Hst.substring_terms("timeout", spec) == [] and Hst.substring_terms(" timeout", spec) == []
        assert Hst.substring_terms(" TimeOut\t", spec) == ["timeout"]


def test_a_separator_spec_splits_partial_whole_partial():
    dash = Tokenizer(" -", lower=True, ngram=3)
    assert Hst.substring_terms("a-bcd-e", dash) == ["bcd"]
    assert Hst.substring_terms("a-bcd-e", dataclasses.replace(dash, ngram=0)) == ["bcd"]
    assert Hst.substring_terms("a-bcdef-e", dash) == ["bcd", "cde", "def"]
    assert Hst.substring_terms("xyz-bc-efg", dash) == ["xyz", "bc", "efg"]
    assert Hst.substring_terms("xyz-bc-efg", dataclasses.replace(dash, ngram=0)) == ["bc"]
    assert Hst.substring_terms("a-b", TRI) == ["a-b"]                     # no separator of THIS spec: one partial word of three runes
    # without Lower an upper-case needle keeps its case
    assert Hst.substring_terms("TimeOut", dataclasses.replace(TRI, lower=False)) == ["Tim", "ime", "meO", "eOu", "Out"]


def test_a_repeated_window_appears_once_in_first_occurrence_order():
    assert Hst.substring_terms("abcabcab", TRI) == ["abc", "bca", "cab"]
    assert Hst.substring_terms(" go go gone", TRI) == ["go", "gon", "one"]


def test_needle_limits():
    for bad, code in ((b"", -1), (b"a\xffb", -1), (b"\xe2\x84", -1), (b"x" * 65, -5), ("é".encode() * 33, -5)):
        with pytest.raises(Hst.HostError) as ei:
            Hst.substring_terms(bad, TRI)
        assert ei.value.code == code, bad
    assert len(Hst.substring_terms("K" * 64, TRI)) == 1              # 192 bytes raw, 64 folded
    with pytest.raises(Hst.HostError):
        Hst.substring_terms("K" * 64, dataclasses.replace(TRI, lower=False))


ALPHABET = list("abcXYZ09") + [" ", " ", "-", ",", ".", "\t", "é", "É", "K", "İ", " ", "\U0001F600"]
PROPERTY_SPECS = {
    "default": WORD,
    "ngram2": dataclasses.replace(WORD, ngram=2),
    "ngram3": TRI,
    "ngram4": dataclasses.replace(WORD, ngram=4),
    "separators": Tokenizer(WHITE_SPACE + "-,.", unicode_space=True, lower=True, ngram=3),
    "separators_words": Tokenizer(WHITE_SPACE + "-,.", unicode_space=False, lower=True),
    "raw": Tokenizer(WHITE_SPACE + "-", unicode_space=True, lower=False, ngram=3),
    "raw_words": Tokenizer(WHITE_SPACE, unicode_space=True, lower=False),
}


@pytest.mark.parametrize("name", sorted(PROPERTY_SPECS))
def test_every_term_of_a_needle_cut_from_a_text_is_a_token_of_the_text(name):
    """>= 20 000 texts over the specs: the needle is a slice, at rune boundaries, of the folded text; a term that is no token of the
    text would be a bloom false negative"""
    spec = PROPERTY_SPECS[name]
    rng = np.random.default_rng(sorted(PROPERTY_SPECS).index(name))
    with_terms = 0
    for _ in range(2600):
        text = "".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=int(rng.integers(1, 28))))
        folded = SR.runes(SR.fold(text, spec))
        a = int(rng.integers(0, len(folded)))
        b = min(len(folded), a + int(rng.integers(1, 16)))
        needle = b"".join(folded[a:b])
        if len(needle) > 64:
            continue
        tokens = set(Hst.tokenize(text, spec, as_bytes=True))
        terms = Hst.substring_terms(needle, spec, as_bytes=True)
        assert set(terms) <= tokens, (text, needle, terms)
        assert len(set(terms)) == len(terms)
        with_terms += bool(terms)
    assert with_terms > 300


def test_the_guard():
    field_and = lambda f, ws: Q.And(*[Q.FieldToken(f, w) for w in ws])
    timeout = ["tim", "ime", "meo", "eou", "out"]
    for guard in (lambda s: Hst.prune_query_sub(None, None, s, TRI), lambda s: Q.substring_guard_bloom_query(s, TRI)):
        assert guard(Q.Substring("timeout")) == Q.And(*[Q.Token(w) for w in timeout])
        assert guard(Q.FieldSubstring("msg", "timeout")) == field_and("msg", timeout)
        assert guard(Q.FieldSubstring("msg", "by")) == Q.Field("msg")                   # a termless field condition: the field must exist
        assert guard(Q.Substring("by")) is None                                          # a termless any-field condition: nil, always true
        # under Or the nil condition stays in its place (never dropped: the Or is true for every block)
        g = guard(Q.SubstringOr(Q.Substring("by"), Q.FieldSubstring("msg", "timeout")))
        assert g == {"ExpressionType": "OR", "Children": [Q.NIL_CONDITION, field_and("msg", timeout)]}
        # under And it leaves the other children
        g = guard(Q.SubstringAnd(Q.Substring("by"), Q.FieldSubstring("msg", "timeout"), Q.FieldSubstring("f", "x")))
        assert g == {"ExpressionType": "AND", "Children": [field_and("msg", timeout), Q.Field("f")]}
        assert guard(Q.SubstringAnd(Q.Substring("by"), Q.Substring("on re"))) is None
        assert guard(None) is None


def test_an_or_with_a_termless_child_prunes_nothing():
    """the pruning expression evaluated as the probe evaluates it (query_exec.go:89-159: nil condition => true) over a block that
    holds none of the windows"""
    g = Hst.prune_query_sub(None, None, Q.SubstringOr(Q.Substring("by"), Q.FieldSubstring("msg", "timeout")), TRI)
    cb = Q.compile_queries([g])
    from bloomsearch_amd._lib import OP_AND, OP_OR, OP_TERM, OP_TRUE
    stack = []
    for o in cb.prog_ops:
        opc, arg = o >> 28, o & 0x0FFFFFFF
        if opc == OP_TERM:
            stack.append(False)                      # the block has no term at all
        elif opc == OP_TRUE:
            stack.append(True)
        elif opc in (OP_AND, OP_OR):
            kids = [stack.pop() for _ in range(arg)]
            stack.append(all(kids) if opc == OP_AND else any(kids))
    assert stack == [True]


def test_the_pruning_expression_joins_three_sides():
    bloom, regex, sub = Q.Token("z"), Q.FieldRegex("a", "b+"), Q.FieldSubstring("msg", "time")
    want = Q.and_bloom_queries(Q.prune_bloom_query(bloom, regex), Q.And(Q.FieldToken("msg", "tim"), Q.FieldToken("msg", "ime")))
    assert Hst.prune_query_sub(bloom, regex, sub, TRI) == want == Q.prune_bloom_query(bloom, regex, sub, TRI)
    assert Hst.prune_query_sub(None, None, sub, WORD) == Q.Field("msg")


@pytest.mark.parametrize("bloom", [None, Q.Token("z"), Q.And(Q.Field("a"), Q.Or(Q.Token("b"), Q.FieldToken("c", "d")))])
@pytest.mark.parametrize("regex", [None, Q.FieldRegex("a", "b+"), Q.RegexOr(Q.FieldRegex("a", "x"), Q.FieldRegex("b.c", "y"))])
def test_a_null_substring_tree_is_bsh_prune_query(bloom, regex):
    assert Hst.prune_query_sub(bloom, regex, None, TRI) == Hst.prune_query(bloom, regex)
    assert Hst.prune_query_sub(bloom, regex, None, None) == Hst.prune_query(bloom, regex)
    assert Q.prune_bloom_query(bloom, regex, None) == Q.prune_bloom_query(bloom, regex)


def test_the_bloom_reader_does_not_know_substring_conditions():
    """"SUBSTRING" is no BloomCondition type: the bloom JSON reader is untouched and an unknown type still means false"""
    e = {"ExpressionType": "CONDITION", "Condition": {"Type": "SUBSTRING", "Field": "", "Token": "abc"}}
    assert Hst.match_row(e, b'{"t":"abc"}') is False
