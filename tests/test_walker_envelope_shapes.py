"""tests/walker_envelope_shapes.py against oracle/walker_oracle.py and, through the host C ABI, the host walker and matcher against the
same oracle and restatements: every shape has the longest path and the depth it claims, every family reaches both sides of the
envelope, in_envelope agrees with the claimed side, the host walker's entry sets are the oracle's for every row (the ones outside the
envelope are the host's to finish), and the host matcher's verdicts are the restatements' for the conditions the GPU tests run.
No GPU."""
import pytest

from bloomsearch_amd import host as Hst
from oracle import walker_oracle as W
from tests import ngram_restatement as NR
from tests import substring_restatement as SR
from tests import walker_envelope_shapes as S

WALKERS = sorted(SR.WALKERS)


def oracle_longest(row: bytes) -> int:
    """the longest path the oracle's walk emits, in bytes (a member's full path is emitted whatever its value; prefixes are shorter)"""
    longest = [0]

    def emit(path, value, is_leaf):
        longest[0] = max(longest[0], len(path.encode("utf-8")))
    W.for_each_path_value(W.parse(row), emit)
    return longest[0]


def bracket_depth(row: bytes) -> int:
    """the most containers open at once, counted over the row's bytes outside its strings"""
    depth = deepest = 0
    in_string = escaped = False
    for c in row.decode("utf-8"):
        if in_string:
            if escaped:
                escaped = False
            elif c == "\\":
                escaped = True
            elif c == '"':
                in_string = False
        elif c == '"':
            in_string = True
        elif c in "{[":
            depth += 1
            deepest = max(deepest, depth)
        elif c in "}]":
            depth -= 1
    assert depth == 0 and not in_string
    return deepest


def test_every_shape_is_what_its_entry_claims():
    names = [s.name for s in S.shapes()]
    assert len(names) == len(set(names))
    for s in S.shapes():
        assert oracle_longest(s.row) == s.longest, s.name
        assert bracket_depth(s.row) == s.depth, s.name
        assert S.measure(s.row) == (s.longest, s.depth), s.name
        assert s.inside == (s.longest <= 96 and s.depth <= 16), s.name
        assert S.in_envelope(s.row) == s.inside, s.name


def test_every_family_reaches_both_sides():
    for family in S.families():
        sides = {s.inside for s in S.shapes() if s.family == family}
        assert sides == {True, False}, family
    at = {(s.longest, s.depth) for s in S.shapes()}
    assert {n for n, _ in at} >= {95, 96, 97} and {d for _, d in at} >= {15, 16, 17}
    assert (96, 16) in at                                                        # both limits at once


def test_the_two_consequences_of_the_rule():
    assert S.in_envelope(('{"%s":{"":1}}' % ("d" * 95)).encode())                  # "parent." is 96 bytes
    assert not S.in_envelope(('{"%s":{"":1}}' % ("g" * 96)).encode())              # a 96-byte parent with any member, an empty key included
    for value in ("1", '"x"', "null", "{}", "[]", "[1,[2]]"):
        assert S.in_envelope(('{"%s":%s}' % ("g" * 96, value)).encode()), value
    by_name = {s.name: s for s in S.shapes()}
    assert by_name["parent_95_child_0"].inside and not by_name["parent_96_child_0"].inside and not by_name["parent_95_child_1"].inside


def test_last_runes_end_at_the_cap_once_and_straddle_it_at_every_later_start():
    for name, text, n in S.LAST_RUNES:
        ends = sorted(s.longest for s in S.shapes() if s.family == "path_last_rune" and s.name.startswith(name + "_ends_at_"))
        assert ends == list(range(96, 96 + max(n, 2))), name
        key = W.parse(('{"%s":0}' % text).encode())[1][0][0]
        assert len(key) == 1 and len(key.encode("utf-8")) == n, name


def test_alignment_rows_start_the_long_key_at_every_alignment():
    at, starts = 0, {96: [], 97: []}
    for row, name, longest in S.alignment_rows():
        assert S.measure(row) == (longest, 1) and oracle_longest(row) == longest
        if longest > 1:
            starts[longest].append(at % 8)
        at += len(row)
    assert starts == {96: list(range(8)), 97: list(range(8))}


def test_the_96_dot_key_has_96_distinct_field_entries():
    by_name = {s.name: s for s in S.shapes()}
    fields = W.index_row(by_name["root_dots96"].row)[0]
    assert fields == {"." * n for n in range(1, 97)}
    # under a parent the parent's joining dot is no prefix of its own: "p." is a field only as the prefix before the key's first dot
    assert W.index_row(by_name["parent_a_dot"].row)[0] == {"p", "p.a", "p.a."}
    assert W.index_row(by_name["parent_dot"].row)[0] == {"p", "p.", "p.."}
    assert W.index_row(by_name["root_dot"].row)[0] == {"."}
    assert W.index_row(by_name["parent_a_dotdot_b"].row)[0] == {"p", "p.a", "p.a.", "p.a..b"}


def test_strip_rows():
    rows = S.strip_rows()
    assert len(rows) >= 513 and all(S.in_envelope(r) for r in rows)
    for i in (255, 256, len(rows) - 1):                                         # the last lane of a workgroup, the first of the next, the last of the launch
        assert S.strip_is_full(i)
    for i, r in enumerate(rows):
        if S.strip_is_full(i):
            assert S.measure(r) == (96, 16) and W.index_row(r)[0] == {S.strip_letter(i) * 96}
            assert not S.strip_is_full(i - 1) or i == 256
        else:
            assert S.measure(r) == (4, 2)
    q = S.strip_query()
    want = [S.reference(r, q) for r in rows]
    assert any(want[i] for i in range(len(rows)) if S.strip_is_full(i)) and any(want[i] for i in range(len(rows)) if not S.strip_is_full(i))
    assert not all(want)


@pytest.mark.parametrize("walker", WALKERS)
def test_the_host_walker_finds_the_oracles_entry_sets(walker):
    tok = SR.WALKERS[walker]
    for row in S.match_rows() + S.strip_rows()[250:260]:
        es = Hst.EntrySets()
        es.index_row(row, tok)
        want = NR.entry_sets([row], SR.spec_of(tok))
        assert es.as_python_sets() == want, row
        if tok is None:
            assert want == W.index_row(row), row


@pytest.mark.parametrize("walker", WALKERS)
def test_the_host_matcher_answers_as_the_restatements_do(walker):
    """bsh_match_row* decide the rows the device hands back, and the Engine test has no other reference for them"""
    tok = SR.WALKERS[walker]
    rows = S.match_rows()
    for q in S.queries(S.token_of(tok)) + [S.strip_query(S.token_of(tok))]:
        seen = set()
        for row in rows + (S.strip_rows()[:40] if q.name == "strip" else ()):
            got = True
            if q.bloom is not None:
                got = got and Hst.match_row(q.bloom, row, tok)
                if tok is None:
                    assert Hst.match_row(q.bloom, row) == W.matches_bloom_expression(row, q.bloom), (q.name, row)
            if q.regex is not None:
                got = got and Hst.match_row_regex(q.regex, row)
            if q.substring is not None:
                got = got and Hst.match_row_substring(q.substring, row, tok)
            if q.range is not None:
                got = got and Hst.match_row_range(q.range, row)
            assert got == S.reference(row, q, tok), (q.name, row)
            if S.in_envelope(row):
                seen.add(got)
        assert seen == {True, False}, q.name                                   # both verdicts among the rows the device decides
