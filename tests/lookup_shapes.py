"""The lookup walker (k_match_rows_lookup*, csrc/match_lookup.hip.h) at the edges of its two probe loops: the table of cases
tests/test_match_lookup_edges_gpu.py runs, condition strings PLACED where a case needs them, restatements of the host's table
arithmetic (host/lookup_plan.hpp) over Python integers, and a plain model of the kernel's rule with a report of the edges a case
touched.  tests/test_lookup_shapes.py keeps this file honest (the restated placement slot for slot against the library's own header
through tests/lookup_plan_check.cpp, every family's property, coverage of every named edge computed from the touch reports, the model's
verdicts against the oracle walker's, and a list of deliberately wrong rules with the first case each breaks).  Test infrastructure only:
no GPU, no call into the library.

Placement.  A string's first slot and tag are functions of word 0 of its base hash: string_slot0 = h0 & (slots - 1), string_tag =
(h0 >> 32) & 0xFFFFF; a table of n strings has the least power of two >= 2n slots, so 1 string lies in 2 slots, 2 in 4, 5..8 in 16
and 1 025..2 048 in 4 096.  The searches reuse tests/table_shapes.py (words, base_hashes_np, hashes): 10-letter lower-case words,
which the default and the separator walkers emit unchanged as a word and as a key; the n-gram walker's tokens are 3-rune windows, so
its shapes come from the 17 576 three-letter words (a word of three runes is its own only window).  Everything a search returns is
hashed again with the oracle's base_hashes and the requested property asserted on that value; no search looks at more than
table_shapes.SEARCH_BUDGET candidates.  A pair's first slot is arithmetic over the two string ids ((fid << 16 | tid) * 0x9E3779B1,
top bits), and ids are given in order of first appearance, so the pair runs are chosen by arithmetic alone: P leading Token conditions
fix the ids 0 .. P - 1, and the FieldToken conditions are picked among the P * P id pairs by their first slot.

Not searchable, and left out: two strings equal in h0 but not in h1..h3 (a 64-bit birthday; the constructed collision pairs share all
four words), ten strings under one tag in one slot of a 4 096-slot table (32 shared bits, ten times), a third string under a tag pair
of the three-letter namespace (none of its 145 shared tags holds three words).  tests/test_match_lookup_plan.py covers those
placements on the CPU with synthetic h0 values.

The model (probe_row) follows the comment block of match_lookup.hip.h: an emission probes the string table from its first slot to the
run's empty slot, wrapping; on a tag hit the four hash words are compared, then the role (a path role for field and leaf requests, a
word role for words), then the fingerprint — "equal fingerprint" is taken as "equal bytes" — and a role-holding string with equal
hashes and other bytes makes the row a handed-back row; the probe goes on behind a match.  A leaf request forgets the leaf's field id,
a leaf path that is some FieldToken's field sets it, and a word that is some FieldToken's token probes the pair table with it.  Rule's
attributes are where the wrong rules differ.  "stop at the table's end instead of at the empty slot" is read as: the loop's only end
is its slot count, an empty slot is compared like any other — its word is tag 0xFFFFF, id 0xFFF, so an emission of that tag reads a
record no string has (the model reports it as `bad_read`).

Cost.  This module's import (every search, every table, every case modelled under its walkers, every property asserted) takes 1.0 s
on the development machine, one core, beside 0.5 s for table_shapes' own import; the searches look at 9.5 M candidates in all, the
two extreme tags (three words of one 20-bit tag each) most of them, so none needed thinning.  tests/test_lookup_shapes.py runs in 6 s
there (the oracle's verdict on every row of every condition is most of it), tests/test_match_lookup_plan.py in 3 s.
"""
from __future__ import annotations

import functools
import itertools
from collections import namedtuple

import numpy as np

from tests import table_shapes as TS

FIELD, TOKEN, FIELD_TOKEN = 0, 1, 2           # host/lookup_plan.hpp kKindField, kKindToken, kKindFieldToken
NO_STRING, NO_COND = 0xFFFFFFFF, 0xFFFF
SLOT_EMPTY, PAIR_EMPTY = 0xFFFFFFFF, (1 << 64) - 1
ID_BITS, ID_MASK = 12, 0xFFF
ROLE_FT_FIELD, ROLE_FT_TOKEN = 1, 2
MAX_CONDS, MAX_STRINGS = 1024, 2048


# ---- host/lookup_plan.hpp, restated over Python integers ----

def table_slots(n: int) -> int:
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def string_slot0(h0: int, slots: int) -> int:
    return h0 & 0xFFFFFFFF & (slots - 1)


def string_tag(h0: int) -> int:
    return (h0 >> 32) & 0xFFFFF


def next_slot(i: int, slots: int) -> int:
    return (i + 1) & (slots - 1)


def place_strings(h0s):
    slots = table_slots(len(h0s))
    tab = [SLOT_EMPTY] * slots
    for sid, h0 in enumerate(h0s):
        i = string_slot0(h0, slots)
        while tab[i] != SLOT_EMPTY:
            i = next_slot(i, slots)
        tab[i] = string_tag(h0) << ID_BITS | sid
    return tab


def pair_key(fid: int, tid: int) -> int:
    return (fid << 16 | tid) & 0xFFFFFFFF


def pair_slot0(key: int, slots: int) -> int:
    return ((key * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def place_pairs(pairs):
    slots = table_slots(len(pairs))
    tab = [PAIR_EMPTY] * slots
    for fid, tid, cond in pairs:
        i = pair_slot0(pair_key(fid, tid), slots)
        while tab[i] != PAIR_EMPTY:
            i = next_slot(i, slots)
        tab[i] = pair_key(fid, tid) << 32 | cond
    return tab


def want_plan(conds, key=str):
    """build_strings restated: ids in order of first appearance in a role; -> (recs as packed words, string_of, canon, pairs,
    pair_cond).  key: what makes two condition strings one string (tests/test_match_lookup_plan.py hands in numbers)"""
    ids, recs, string_of, canon, pairs, pair_cond = {}, [], [], [], [], {}

    def sid(s, entry):
        if s not in ids:
            ids[s] = len(recs)
            recs.append([entry, NO_COND, NO_COND, 0])
        return ids[s]

    for c, (kind, f, t) in enumerate(conds):
        fid = sid(key(f), 2 * c) if kind != TOKEN else NO_STRING
        tid = sid(key(t), 2 * c + 1) if kind != FIELD else NO_STRING
        string_of += [fid, tid]
        if kind == FIELD:
            if recs[fid][1] == NO_COND:
                recs[fid][1] = c
            canon.append(recs[fid][1])
        elif kind == TOKEN:
            if recs[tid][2] == NO_COND:
                recs[tid][2] = c
            canon.append(recs[tid][2])
        else:
            if (fid, tid) not in pair_cond:
                pair_cond[(fid, tid)] = c
                pairs.append((fid, tid, c))
                recs[fid][3] |= 1
                recs[tid][3] |= 2
            canon.append(pair_cond[(fid, tid)])
    return [e | fc << 16 | tc << 32 | fl << 48 for e, fc, tc, fl in recs], string_of, canon, pairs, pair_cond


class Table:
    """what the host hands the walker for a list of (kind, field bytes, token bytes) conditions"""

    def __init__(self, conds):
        self.conds = tuple(conds)
        assert len(self.conds) <= MAX_CONDS
        self.recs, self.string_of, self.canon, self.pairs, self.pair_cond = want_plan(self.conds, key=bytes)
        flat = [s for _, f, t in self.conds for s in (f, t)]
        self.strings = [flat[r & 0xFFFF] for r in self.recs]                           # by id: the bytes of the record's entry
        assert len(set(self.strings)) == len(self.strings) <= MAX_STRINGS
        self.hashes = [TS.hashes(s) for s in self.strings]
        self.str_slots = place_strings([h[0] for h in self.hashes])
        self.pair_slots = place_pairs(self.pairs)

    def slot0_of(self, s: bytes) -> int:
        return string_slot0(TS.hashes(s)[0], len(self.str_slots))


# ---- the kernel's rule ----

class Rule:
    """The rule as written.  The attributes are where the wrong rules differ."""
    name = "as written"
    first_tag_hit_ends = False       # (wrong) the probe ends behind the first tag hit, whatever it was
    tag_hit_is_match = False         # (wrong) a tag hit is taken for the string: no compare of the hash words or the fingerprint
    string_wrap = True               # the string probe wraps by & (slots - 1); (wrong) it ends behind the last slot
    pair_wrap = True                 # the same of the pair probe
    end_at_empty = True              # an empty slot ends the probe; (wrong) only the slot count does
    role_test = True                 # (wrong) every string is compared with every kind of emission
    fingerprint_first = False        # (wrong) the fingerprint is compared before the role is looked at
    break_behind_match = False       # (wrong) the probe ends behind a match
    leaf_reset = "leaf"              # the leaf's field id is forgotten at a leaf request; (wrong) "never", "field"
    pair_ids_swapped = False         # (wrong) the probe's pair key is (token id, field id)
    flag_shift = 6                   # the flag word of condition c is c >> 6; (wrong) 5


def wrong(name, **changes):
    return type("Wrong", (Rule,), dict(changes, name=name))


WRONG_RULES = (
    wrong("stop at the first tag hit", first_tag_hit_ends=True),
    wrong("take a tag hit as a match", tag_hit_is_match=True),
    wrong("no wrap in the string table", string_wrap=False),
    wrong("no wrap in the pair table", pair_wrap=False),
    wrong("stop at the table's end instead of at the empty slot", end_at_empty=False),
    wrong("skip the role test", role_test=False),
    wrong("fingerprint before role", fingerprint_first=True),
    wrong("break behind a match", break_behind_match=True),
    wrong("leaf_fid not reset at a leaf request", leaf_reset="never"),
    wrong("leaf_fid reset at a field request only", leaf_reset="field"),
    wrong("pair key with the ids swapped", pair_ids_swapped=True),
    wrong("flag word index c >> 5", flag_shift=5),
)

# every edge a case can touch; tests/test_lookup_shapes.py asserts each is touched by some case
EDGES = (
    "tables-empty",                  # a probe of a table without strings: the first slot is empty
    "tag-hit-other-record",          # a tag hit whose hash words differ: the probe goes on
    "match-behind-tag-hit",          # ... and finds the emission's own string behind it
    "miss-behind-tag-hit",           # ... and ends at the empty slot: an absent twin
    "two-tag-hits-then-miss",        # an absent string behind two strings of its tag
    "match-behind-two-tag-hits",     # the third of three strings under one tag in one run
    "tag-0xFFFFF-hit", "tag-0xFFFFF-twin", "tag-0-hit", "tag-0-twin",
    "occupied-behind-match",         # the probe looks at a further occupied slot behind a match
    "collision",                     # equal hash words, a role for this emission, other bytes: handed back
    "collision-behind-match",        # ... found behind the emission's own string
    "match-behind-collision",        # ... and the other way round
    "collision-behind-wrap",         # ... in a slot reached by wrapping
    "role-filtered-path",            # equal hash words, a path emission, a string without a path role
    "role-filtered-word",            # equal hash words, a word, a string without a word role
    "role-filtered-other-bytes",     # ... of other bytes: the role test precedes the fingerprint
    "string-wrap",                   # a probe steps from the last slot to slot 0
    "match-behind-wrap",             # a string found in a slot reached by wrapping
    "miss-across-wrap",              # an absent string's probe wraps and ends at the empty slot behind it
    "miss-from-slot-0",              # an absent string whose first slot is slot 0, occupied by a wrapped run
    "run-60",                        # a probe over 60 occupied slots or more
    "slots-2", "slots-4", "slots-16", "slots-4096",
    "string-id-0", "string-id-2047",
    "leaf-sets-fid", "leaf-resets-fid", "null-leaf-sets-fid", "word-without-fid", "word-role-without-pair-role",
    "pair-hit", "pair-hit-behind-other", "pair-miss-at-empty", "pair-miss-behind-run", "pair-wrap", "pair-hit-behind-wrap",
    "pair-miss-across-wrap", "pair-slots-2", "pair-slots-4", "pair-slots-16", "pair-slots-2048",
    "field-token-and-pair-from-one-leaf",
    "cond-0", "cond-63", "cond-64", "cond-1023", "flag-word-15-bit-63",
)

Verdict = namedtuple("Verdict", "bits handed_back bad_read touched")


def probe_row(tab: Table, emissions, rule=Rule) -> Verdict:
    """emissions: [(request, bytes)], request "field" (a path that is no leaf's), "leaf", "null-leaf" or "word", in walk order
    -> (bool per condition, handed back, did the rule read a record no string has, the edges touched)"""
    S, P = len(tab.str_slots), len(tab.pair_slots)
    flags, touched = set(), set()
    collided = bad_read = False
    leaf_fid, leaf_field_cond = None, False
    touched.add("slots-%d" % S)

    def set_flag(c):
        flags.add((c >> rule.flag_shift, c & 63))
        for e, at in (("cond-0", 0), ("cond-63", 63), ("cond-64", 64), ("cond-1023", 1023)):
            if c == at:
                touched.add(e)
        if (c >> 6, c & 63) == (15, 63):
            touched.add("flag-word-15-bit-63")

    def probe_pair(fid, tid, beside):
        key = pair_key(tid, fid) if rule.pair_ids_swapped else pair_key(fid, tid)
        j, passed, wrapped = pair_slot0(key, P), 0, False
        touched.add("pair-slots-%d" % P)
        for _ in range(P):
            if j >= P:
                return
            ps = tab.pair_slots[j]
            if ps == PAIR_EMPTY:
                touched.add("pair-miss-behind-run" if passed else "pair-miss-at-empty")
                if wrapped:
                    touched.add("pair-miss-across-wrap")
                return
            if ps >> 32 == key:
                set_flag(ps & 0xFFFFFFFF)
                touched.add("pair-hit")
                if beside:
                    touched.add("field-token-and-pair-from-one-leaf")
                if passed:
                    touched.add("pair-hit-behind-other")
                if wrapped:
                    touched.add("pair-hit-behind-wrap")
                return
            passed += 1
            if j == P - 1:
                wrapped = True
                touched.add("pair-wrap")
            j = next_slot(j, P) if rule.pair_wrap else j + 1

    for request, s in emissions:
        is_path = request != "word"
        if (request in ("leaf", "null-leaf") and rule.leaf_reset == "leaf") or (request == "field" and rule.leaf_reset == "field"):
            if leaf_fid is not None:
                touched.add("leaf-resets-fid")
            leaf_fid = None
        if request != "word":
            leaf_field_cond = False
        h = TS.hashes(s)
        tag, i = string_tag(h[0]), string_slot0(h[0], S)
        first = i
        others = matched = collisions = passed = 0      # tag hits on other records, matches, collisions, occupied slots seen
        wrapped = False
        for _ in range(S):
            if i >= S:
                break
            slot = tab.str_slots[i]
            if slot == SLOT_EMPTY and rule.end_at_empty:
                if matched == 0 and collisions == 0:
                    if S == 2 and not tab.strings:
                        touched.add("tables-empty")
                    if others == 1:
                        touched.add("miss-behind-tag-hit")
                    if others >= 2:
                        touched.add("two-tag-hits-then-miss")
                    if others and tag in (0, 0xFFFFF):
                        touched.add("tag-0x%X-twin" % tag if tag else "tag-0-twin")
                    if wrapped:
                        touched.add("miss-across-wrap")
                    if first == 0 and passed and tab.slot0_of(tab.strings[tab.str_slots[0] & ID_MASK]) != 0:
                        touched.add("miss-from-slot-0")
                if passed >= 60:
                    touched.add("run-60")
                break
            if matched and slot != SLOT_EMPTY:
                touched.add("occupied-behind-match")
            step = True
            if slot >> ID_BITS == tag:
                sid = slot & ID_MASK
                if sid >= len(tab.recs):
                    bad_read = True                       # the empty slot's word read as a string: no such record
                else:
                    rec = tab.recs[sid]
                    fc, tc, fl = rec >> 16 & 0xFFFF, rec >> 32 & 0xFFFF, rec >> 48
                    same_hashes = rule.tag_hit_is_match or tab.hashes[sid] == h
                    same_bytes = rule.tag_hit_is_match or tab.strings[sid] == s
                    role = (fc != NO_COND or fl & ROLE_FT_FIELD) if is_path else (tc != NO_COND or fl & ROLE_FT_TOKEN)
                    if not same_hashes:
                        others += 1
                        touched.add("tag-hit-other-record")
                    elif rule.fingerprint_first and not same_bytes:
                        collided = True
                    elif rule.role_test and not role:
                        touched.add("role-filtered-path" if is_path else "role-filtered-word")
                        if not same_bytes:
                            touched.add("role-filtered-other-bytes")
                    elif not same_bytes:
                        collided = True
                        collisions += 1
                        touched.add("collision")
                        if matched:
                            touched.add("collision-behind-match")
                        if wrapped:
                            touched.add("collision-behind-wrap")
                    else:
                        matched += 1
                        if others == 1:
                            touched.add("match-behind-tag-hit")
                        if others >= 2:
                            touched.add("match-behind-two-tag-hits")
                        if collisions:
                            touched.add("match-behind-collision")
                        if wrapped:
                            touched.add("match-behind-wrap")
                        if tag in (0, 0xFFFFF):
                            touched.add("tag-0x%X-hit" % tag if tag else "tag-0-hit")
                        if sid in (0, MAX_STRINGS - 1):
                            touched.add("string-id-%d" % sid)
                        c = fc if is_path else tc
                        if c != NO_COND:
                            set_flag(c)
                            if request == "leaf":
                                leaf_field_cond = True
                        if request in ("leaf", "null-leaf") and fl & ROLE_FT_FIELD:
                            leaf_fid = sid
                            touched.add("leaf-sets-fid" if request == "leaf" else "null-leaf-sets-fid")
                        if request == "word":
                            if fl & ROLE_FT_TOKEN and leaf_fid is not None:
                                probe_pair(leaf_fid, sid, leaf_field_cond and tc != NO_COND)
                            elif fl & ROLE_FT_TOKEN:
                                touched.add("word-without-fid")
                            else:
                                touched.add("word-role-without-pair-role")
                        if rule.break_behind_match:
                            step = False
                    if rule.first_tag_hit_ends:
                        step = False
            if not step:
                break
            passed += 1
            if i == S - 1:
                wrapped = True
                touched.add("string-wrap")
            i = next_slot(i, S) if rule.string_wrap else i + 1
    bits = [(tab.canon[c] >> 6, tab.canon[c] & 63) in flags for c in range(len(tab.conds))]
    return Verdict(tuple(bits), collided, bad_read, frozenset(touched))


# ---- emissions of a row under the three walkers ----

WALKERS = ("default", "separator", "trigram")


def spec_of(walker: str):
    """the tokenizer spec the GPU test hands the call (None: the default walker)"""
    if walker == "default":
        return None
    from tests import ngram_restatement as G, tokenizer_restatement as R
    return R.SPECS["punct_lower"] if walker == "separator" else G.SPECS["tri_default"]


@functools.lru_cache(maxsize=None)
def emissions(row: bytes, walker: str):
    """the requests the walker makes for the row, in walk order.  default: the oracle walker's paths and its tokenizer; separator and
    trigram: tests/tokenizer_restatement.py's leaves with that file's, or tests/ngram_restatement.py's, tokens"""
    from oracle import walker_oracle as W
    out = []
    if walker == "default":
        def emit(path, value, is_leaf):
            text = W.leaf_token_input(value) if is_leaf else None
            out.append(("field" if not is_leaf else "leaf" if text is not None else "null-leaf", path.encode()))
            if text is not None:
                out.extend(("word", t.encode()) for t in W.basic_whitespace_lower_tokenizer(text))
        W.for_each_path_value(W.parse(row), emit)
        return tuple(out)
    from tests import ngram_restatement as G, tokenizer_restatement as R
    spec = spec_of(walker)
    for path, is_leaf, text in R.leaves(row):
        out.append(("field" if not is_leaf else "leaf" if text is not None else "null-leaf", path.encode()))
        if text is not None:
            out.extend(("word", t) for t in (R.tokens(text, spec) if walker == "separator" else G.tokens(text, spec)))
    return tuple(out)


# ---- searches ----

SHORT_LEN = 3


@functools.lru_cache(maxsize=None)
def short_words() -> np.ndarray:
    """u8 [17 576][3]: every three-letter lower-case word"""
    v = np.arange(26 ** SHORT_LEN)
    return np.stack([ord("a") + (v // 26 ** (SHORT_LEN - 1 - k)) % 26 for k in range(SHORT_LEN)], axis=1).astype(np.uint8)


SEARCHED = [0]                    # candidates looked at, in all


def _batches(ns: str):
    """(words u8 [n][L], h0 u64 [n]) of a namespace: "short", or the two-letter tag of a 10-letter namespace"""
    if ns == "short":
        SEARCHED[0] += len(short_words())
        yield short_words(), TS.base_hashes_np(short_words())[0]
        return
    first = 0
    while first < TS.SEARCH_BUDGET:
        w = TS.words(ns, first, TS.SEARCH_BATCH)
        SEARCHED[0] += len(w)
        yield w, TS.base_hashes_np(w)[0]
        first += TS.SEARCH_BATCH


def _np_slot0(h0, slots):
    return (h0 & np.uint64(slots - 1)).astype(np.int64)


def _np_tag(h0):
    return ((h0 >> np.uint64(32)) & np.uint64(0xFFFFF)).astype(np.int64)


def pick(ns: str, n: int, slots: int = 2, slot0=None, tag=None, avoid=()):
    """the first n words of the namespace whose first slot (of `slots`) and tag are the given ones and which are not in `avoid`"""
    found = []
    for w, h0 in _batches(ns):
        ok = np.ones(len(w), dtype=bool)
        if slot0 is not None:
            ok &= _np_slot0(h0, slots) == slot0
        if tag is not None:
            ok &= _np_tag(h0) == tag
        for j in np.flatnonzero(ok):
            s = w[j].tobytes()
            if s not in avoid:
                found.append(s)
                if len(found) == n:
                    break
        if len(found) == n:
            break
    else:
        raise LookupError("pick(%s): %d of %d words" % (ns, len(found), n))
    for s in found:                                                                     # again, through the oracle's hash
        h0 = TS.hashes(s)[0]
        assert s.isalpha() and s.islower() and len(s) in (SHORT_LEN, TS.WORD_LEN)
        assert slot0 is None or string_slot0(h0, slots) == slot0, s
        assert tag is None or string_tag(h0) == tag, s
    assert len(set(found)) == n
    return tuple(found)


def tag_groups(ns: str, size: int, slots: int, count: int = 1, slot0=None, avoid=()):
    """`count` disjoint groups of `size` words with one tag and one first slot of `slots` (a birthday search over tag and slot bits)"""
    seen_w, seen_k = [], []
    for w, h0 in _batches(ns):
        keep = np.ones(len(w), dtype=bool) if slot0 is None else _np_slot0(h0, slots) == slot0
        seen_w.append(w[keep])
        seen_k.append(_np_tag(h0[keep]) * slots + _np_slot0(h0[keep], slots))
        words, keys = np.concatenate(seen_w), np.concatenate(seen_k)
        order = np.argsort(keys, kind="stable")
        uniq, start, counts = np.unique(keys[order], return_index=True, return_counts=True)
        groups = []
        for at in np.flatnonzero(counts >= size):
            g = [words[order[start[at] + k]].tobytes() for k in range(counts[at])]
            g = [s for s in g if s not in avoid][:size]
            if len(g) == size:
                groups.append(tuple(g))
        if len(groups) >= count:
            groups = sorted(groups)[:count]
            for g in groups:
                hs = [TS.hashes(s)[0] for s in g]
                assert len(set(g)) == size and len({string_tag(h) for h in hs}) == 1 and len({string_slot0(h, slots) for h in hs}) == 1
                assert slot0 is None or string_slot0(hs[0], slots) == slot0
            return groups
    raise LookupError("tag_groups(%s): fewer than %d groups of %d" % (ns, count, size))


def fillers(ns: str, n: int, avoid=()):
    """n words of the namespace as they come (natural strings: no placement asked)"""
    return pick(ns if ns == "short" else "z" + ns[1], n, avoid=avoid)


# ---- the table of cases ----

# conds: (kind, field bytes, token bytes) in table order.  rows: bytes.  composites: expressions over condition indices — an int (TERM
# c), None (the nil expression), ("AND", ...) or ("OR", ...).  handed_back: the rows only the host can decide.  walkers: which
# instances run it.  why: the family's property, one line.  A condition string need not be text (the collision partner is not).
Case = namedtuple("Case", "name family conds rows composites handed_back walkers why")

LONG_WALKERS, SHORT_WALKERS = ("default", "separator"), ("trigram",)


def obj(*members) -> bytes:
    """a row of string members: obj(("k", "v w"), ...); a value that is no bytes goes in as a JSON literal"""
    parts = []
    for k, v in members:
        parts.append(b'"' + k + b'":' + (b'"' + v + b'"' if isinstance(v, bytes) else str(v).encode()))
    return b"{" + b",".join(parts) + b"}"


def word_row(*words) -> bytes:
    return obj((b"k", b" ".join(words)))


def T(s):
    return (TOKEN, b"", s)


def F(s):
    return (FIELD, s, b"")


def FT(f, t):
    return (FIELD_TOKEN, f, t)


def comp_value(comp, bits):
    """a composite's value from the conditions' truths"""
    if comp is None:
        return True
    if isinstance(comp, int):
        return bool(bits[comp])
    kids = [comp_value(k, bits) for k in comp[1:]]
    return all(kids) if comp[0] == "AND" else any(kids)


def _walkers(ns):
    return SHORT_WALKERS if ns == "short" else LONG_WALKERS


def _sfx(ns):
    return "-3" if ns == "short" else ""


def family_empty_table():
    """no condition at all: no string, two empty slots in each table; the queries are the nil expression, And() and Or()"""
    rows = (word_row(b"abc"), obj((b"abc", b"def ghi")), obj((b"a", 7), (b"b", "null")), b"{}")
    return [Case("empty-table", "empty_table", (), rows, (None, ("AND",), ("OR",)), (), WALKERS, family_empty_table.__doc__)]


def family_tag_twin_absent(ns):
    """a != b with one tag and one first slot, only a in the table: b meets a's tag, differs in the hash words, and misses"""
    (a, b), = tag_groups(ns, 2, 4, avoid=())
    n, c = fillers(ns, 2, avoid=(a, b))
    out = []
    for slots, extra in ((2, ()), (4, (c,))):
        why = family_tag_twin_absent.__doc__ + " (%d slots)" % slots
        rows = (word_row(b), word_row(a), word_row(a, b), word_row(b, a), word_row(n))
        out.append(Case("twin-absent-token-%d%s" % (slots, _sfx(ns)), "tag_twin_absent", tuple(T(s) for s in (a,) + extra), rows, (("OR", 0, 0),),
                        (), _walkers(ns), why))
        rows = (obj((b, n)), obj((a, n)), obj((a, n), (b, n)), obj((b, n), (a, n)), obj((n, n)))       # the twin arrives as a key
        out.append(Case("twin-absent-field-%d%s" % (slots, _sfx(ns)), "tag_twin_absent", tuple(F(s) for s in (a,) + extra), rows, (("AND", 0),),
                        (), _walkers(ns), why))
    return out


def family_tag_twins_present(ns):
    """a, b (and d) with one tag and one first slot, a and b both in a 4-slot table in both orders: each is found, one of them behind
    the other's tag hit; d, absent, probes behind both; all three in one run of an 8-slot table"""
    out = []
    if ns == "short":
        (a, b), = tag_groups(ns, 2, 4)
        d = None
    else:
        (a, b, d), = tag_groups(ns, 3, 8)
    n, = fillers(ns, 1, avoid=(a, b, d))
    rows = [word_row(a), word_row(b), word_row(a, b), word_row(n), obj((a, b))]
    if d:
        rows += [word_row(d), word_row(d, b, a)]
    for name, order in (("ab", (a, b)), ("ba", (b, a))):
        out.append(Case("twins-present-%s%s" % (name, _sfx(ns)), "tag_twins_present", tuple(T(s) for s in order), tuple(rows),
                        (("AND", 0, 1), ("OR", 0, 1)), (), _walkers(ns), family_tag_twins_present.__doc__))
    if d:
        rows += [word_row(d, n), obj((d, a))]
        out.append(Case("triple-present", "tag_twins_present", (T(a), T(b), T(d)), tuple(rows), (("AND", 0, 1, 2), ("OR", 1, 2)), (),
                        _walkers(ns), family_tag_twins_present.__doc__))
    return out


def family_tag_extremes():
    """a string of tag 0xFFFFF (its slot word is one id short of the empty mark) and one of tag 0, each present and hit, each with an
    absent twin of its tag and first slot"""
    out = []
    for tag, name in ((0xFFFFF, "tag-max"), (0, "tag-zero")):
        three = pick("x" + name[4], 3, tag=tag)
        p, q = next((u, v) for u, v in itertools.combinations(three, 2) if (TS.hashes(u)[0] ^ TS.hashes(v)[0]) & 1 == 0)
        rows = (word_row(p), word_row(q), word_row(q, p), obj((p, q)), obj((q, p)))
        out.append(Case(name, "tag_extremes", (T(p),), rows, (), (), LONG_WALKERS, family_tag_extremes.__doc__))
    return out


def family_run_wrap(ns):
    """two or more strings whose first slot is the table's last: the run continues at slot 0; a row for each, an absent word that
    walks across the wrap to the empty slot, and an absent word whose first slot is slot 0"""
    out = []
    for slots in (4, 16) if ns == "short" else (4, 16, 4096):
        n_run = 2 if slots == 4 else 3
        run = pick(ns if ns == "short" else "ra", n_run + 1, slots, slots - 1)
        zero, = pick(ns if ns == "short" else "rb", 1, slots, 0, avoid=run)
        run, absent = run[:n_run], run[n_run]
        if slots == 4:
            conds = [T(s) for s in run]
        elif slots == 16:
            conds = [T(s) for s in run] + [T(s) for s in fillers(ns, 3, avoid=run + (absent, zero))]
        else:
            fill = fillers(ns, 1040, avoid=run + (absent, zero))
            conds = [T(s) for s in run] + [FT(fill[2 * k], fill[2 * k + 1]) for k in range(520)]
        rows = [word_row(s) for s in run] + [word_row(absent), word_row(zero), word_row(*run), obj((run[-1], absent)), obj((absent, run[0]))]
        if slots == 4096:
            rows += [obj((fill[2 * k], fill[2 * k + 1])) for k in (0, 1, 519)] + [obj((fill[0], fill[3]))]
        out.append(Case("run-wrap-%d%s" % (slots, _sfx(ns)), "run_wrap", tuple(conds), tuple(rows), (("OR",) + tuple(range(n_run)),), (),
                        _walkers(ns), family_run_wrap.__doc__))
    return out


LONG_RUN = 60
LONG_RUN_CONDS = (0, 63, 64) + tuple(range(100, 100 + LONG_RUN - 4)) + (1023,)      # the conditions whose tokens form the run


def family_long_run():
    """1 024 FieldToken conditions on 2 048 distinct strings, both tables at their largest; 60 tokens share first slot 4 095, their run
    wraps through slot 0 and on; rows hit its first, a middle and its last string, an absent word of that slot walks all of it; the
    pairs of conditions 0, 63, 64 and 1 023 and string ids 0 and 2 047 are hit"""
    run = pick("la", LONG_RUN + 1, 4096, 4095)
    run, absent = run[:LONG_RUN], run[LONG_RUN]
    fill = iter([s for s in fillers("lb", 2100) if string_slot0(TS.hashes(s)[0], 4096) != 4095][: 2048 - LONG_RUN])
    of_cond = dict(zip(LONG_RUN_CONDS, run))
    conds = [FT(next(fill), of_cond[c] if c in of_cond else next(fill)) for c in range(1024)]
    hit = [0, 63, 64, 1023, LONG_RUN_CONDS[LONG_RUN // 2], 1, 62, 65, 500, 1022]
    rows = [obj((conds[c][1], conds[c][2])) for c in hit]
    rows += [word_row(absent), obj((conds[0][1], absent)), obj((conds[0][1], conds[63][2])), obj((conds[63][1], conds[0][2])),
             obj((conds[1023][2], conds[1023][1])), word_row(*(conds[c][2] for c in LONG_RUN_CONDS[:8])),
             obj((conds[0][1], b" ".join(conds[c][2] for c in (63, 0, 1023)))), obj((conds[64][1], b"q"), (conds[63][1], conds[64][2]))]
    comps = (("OR", 0, 1023), ("AND", 63, 64), ("OR", ("AND", 0, 63), 64))
    return [Case("long-run", "long_run", tuple(conds), tuple(rows), comps, (), LONG_WALKERS, family_long_run.__doc__)]


def family_roles_in_one_run(ns):
    """a path-only string p and a word-only string w with one first slot: p as a word and w as a key hit nothing and hand nothing back;
    and one string in all four roles (Field, Token, a FieldToken's field, a FieldToken's token)"""
    p, w = pick(ns if ns == "short" else "oa", 2, 4, 2)
    s, x, y, n = fillers(ns, 4, avoid=(p, w))
    out = [Case("roles-one-run" + _sfx(ns), "roles_in_one_run", (F(p), T(w)),
                (word_row(p), obj((w, n)), obj((p, w)), obj((w, p)), obj((p, n), (w, p)), word_row(n)), (("AND", 0, 1), ("OR", 0, 1)), (),
                _walkers(ns), family_roles_in_one_run.__doc__)]
    conds = (F(s), T(s), FT(s, x), FT(y, s), FT(s, s))
    rows = (obj((s, s)), obj((y, s)), obj((s, x)), obj((x, s)), obj((y, x)), obj((n, s), (s, n)))
    out.append(Case("four-roles" + _sfx(ns), "roles_in_one_run", conds, rows, (("AND", 0, 1, 4), ("OR", 2, 3)), (), _walkers(ns),
                    family_roles_in_one_run.__doc__))
    return out


PUNCT_SEPARATORS = b" \t\n\v\f\r,;:=/.-\"[]()"        # tests/tokenizer_restatement.py PUNCT: the separator walker must emit a whole


def wrap_collision_pair():
    """tests.test_collisions.pair(seed), the first seed whose a holds no separator of the separator spec and whose first slot is the
    last of a 4-slot table"""
    from tests.test_collisions import pair
    for seed in range(4000):
        a, b = pair(seed)
        if not any(ch in PUNCT_SEPARATORS for ch in a) and string_slot0(TS.hashes(a)[0], 4) == 3:
            assert TS.hashes(a) == TS.hashes(b) and a != b
            return a, b
    raise LookupError("no collision pair")


def family_collision_behind_the_wrap():
    """a and b share all four hash words; the table holds b and a string x of b's first slot, the last of four, so one of the two lies at
    slot 0 behind the wrap: a row holding a is handed back in both orders; with b in a path-only role a word a is not (the role test
    precedes the fingerprint) while a key a is; with a AND b in the table a row holding either is handed back in both orders"""
    a, b = wrap_collision_pair()
    x, = pick("ca", 1, 4, 3)
    n, = fillers("cb", 1, avoid=(x,))
    rows = (word_row(a), word_row(x), word_row(n), word_row(n, a), obj((a, 1)), obj((x, n)))
    why = family_collision_behind_the_wrap.__doc__
    out = []
    for name, conds in (("xb", (T(x), T(b))), ("bx", (T(b), T(x)))):
        out.append(Case("collision-wrap-" + name, "collision_behind_the_wrap", conds, rows, (("OR", 0, 1),), (0, 3), LONG_WALKERS, why))
    out.append(Case("collision-path-only", "collision_behind_the_wrap", (T(x), F(b)), rows, (("OR", 0, 1),), (4,), LONG_WALKERS, why))
    for name, conds in (("ab", (T(a), T(b))), ("ba", (T(b), T(a)))):
        out.append(Case("collision-both-" + name, "collision_behind_the_wrap", conds, rows, (), (0, 3), LONG_WALKERS, why))
    return out


def _pair_slots_of(P, pslots):
    by_slot = {}
    for i in range(P):
        for j in range(P):
            by_slot.setdefault(pair_slot0(pair_key(i, j), pslots), []).append((i, j))
    return by_slot


def family_pair_runs(ns):
    """FieldToken conditions whose pairs' first slots coincide, chosen by arithmetic over the ids: a run that begins at the pair
    table's last slot and wraps, rows for its first and last pair, an absent pair of present strings whose first slot is the run's
    first, the swapped pair of strings that hold both roles, and (f1, t1), (f2, t2) with the row {"f1": "t2"}"""
    out = []
    why = family_pair_runs.__doc__
    for pslots in (2, 4, 16, 2048):
        P = {2: 2, 4: 16, 16: 16, 2048: 128}[pslots]
        s = fillers(ns, P + 1)
        s, n = s[:P], s[P]
        at_last = _pair_slots_of(P, pslots)[pslots - 1]
        row = lambda p: obj((s[p[0]], s[p[1]]))
        if pslots == 2:
            run, absent, fill = [at_last[0]], None, []
        elif pslots == 2048:
            run, absent = at_last[:-1], at_last[-1]
            assert len(run) >= 4
            fill, taken, k = [], set(at_last), 0
            while len(run) + len(fill) < MAX_CONDS - P:                                  # every string a field and a token of some pair
                mult = 2 * k + 7
                for i in range(P):
                    p = (i, (i * mult + 3 + k) % P)
                    if p not in taken and len(run) + len(fill) < MAX_CONDS - P:
                        taken.add(p)
                        fill.append(p)
                k += 1
        else:
            c1, c2, absent = next((u, v, (u[0], v[1])) for u in at_last for v in at_last
                                  if u[0] != v[0] and u[1] != v[1] and (u[0], v[1]) in at_last and len({u[0], u[1], v[0], v[1]}) == 4)
            run = [c1, c2]
            fill = []
            if pslots == 16:
                run.append(next(p for p in at_last if p not in (c1, c2, absent)))
                fill = [(c1[1], c2[0]), (c2[1], c1[0]), (c2[1], c2[1])]                  # t1 a field, f1 a token
                assert not set(fill) & set(run + [absent])
        pairs = fill[: len(fill) // 2] + run + fill[len(fill) // 2:]
        conds = [T(w) for w in s] + [FT(s[i], s[j]) for i, j in pairs]
        assert table_slots(len(pairs)) == pslots
        rows = [row(run[0]), row(run[-1]), obj((s[run[0][0]], n)), obj((n, s[run[0][1]])), word_row(s[run[0][1]])]
        if absent:
            rows += [row(absent), row((run[0][0], run[-1][1])), row((run[0][1], run[0][0]))]
        if fill:
            rows += [row(fill[0]), row(fill[-1]), row((fill[0][1], fill[0][0]))]
        first_pair = P + pairs.index(run[0])
        comps = (("OR", first_pair, P + pairs.index(run[-1])), ("AND", first_pair, run[0][1]))
        out.append(Case("pair-runs-%d%s" % (pslots, _sfx(ns)), "pair_runs", tuple(conds), tuple(rows), comps, (), _walkers(ns), why))
    return out


def family_one_leaf():
    """the lifetime of the leaf's field id, for FieldToken(a, x): the pair holds at ONE leaf — across an array's elements, never across
    leaves, objects, keys or a null; beside Field(a) and Token(x) all three flags come from one leaf"""
    rows = (b'{"a":["q","x"]}', b'{"a":"q","b":"x"}', b'{"a":"q","b":{"c":"x"}}', b'{"a":{"b":"x"}}', b'{"a":"q","":"x"}', b'{"b":"x","a":"q"}',
            b'{"a":"q x"}', b'{"a":"q","a":"x"}', b'{"a":7,"b":"x"}', b'{"a":null,"b":"x"}', b'{"a":"x"}')
    return [Case("one-leaf", "one_leaf", (FT(b"a", b"x"), F(b"a"), T(b"x")), rows, (("AND", 0, 1, 2), ("OR", 0, 2)), (), WALKERS,
                 family_one_leaf.__doc__)]


def _table():
    cases = family_empty_table()
    for ns in ("ta", "short"):
        cases += family_tag_twin_absent(ns) + family_tag_twins_present(ns)
    cases += family_tag_extremes()
    for ns in ("ra", "short"):
        cases += family_run_wrap(ns)
    cases += family_long_run()
    for ns in ("oa", "short"):
        cases += family_roles_in_one_run(ns)
    cases += family_collision_behind_the_wrap()
    for ns in ("pa", "short"):
        cases += family_pair_runs(ns)
    cases += family_one_leaf()
    table = {c.name: c for c in cases}
    assert len(table) == len(cases)
    return table


CASES = _table()
FAMILIES = ("empty_table", "tag_twin_absent", "tag_twins_present", "tag_extremes", "run_wrap", "long_run", "roles_in_one_run",
            "collision_behind_the_wrap", "pair_runs", "one_leaf")
# the families the trigram walker's three-letter namespace can build
TRIGRAM_FAMILIES = ("empty_table", "tag_twin_absent", "tag_twins_present", "run_wrap", "roles_in_one_run", "pair_runs", "one_leaf")


@functools.lru_cache(maxsize=None)
def table_of(name: str) -> Table:
    return Table(CASES[name].conds)


@functools.lru_cache(maxsize=None)
def modelled(name: str, walker: str, rule=Rule):
    """the model's verdict on every row of the case under one walker"""
    case = CASES[name]
    return tuple(probe_row(table_of(name), emissions(r, walker), rule) for r in case.rows)


def touched(name: str):
    """the edges the case touches, under the walkers that run it"""
    return frozenset().union(*[v.touched for w in CASES[name].walkers for v in modelled(name, w)])


# ---- every family's property, asserted through the model ----

def _assert_properties():
    for case in CASES.values():
        tab = table_of(case.name)
        for w in case.walkers:
            vs = modelled(case.name, w)
            assert [r for r, v in enumerate(vs) if v.handed_back] == list(case.handed_back), case.name
            assert not any(v.bad_read for v in vs), case.name
            assert (case.family == "collision_behind_the_wrap") == bool(case.handed_back), case.name
        t = touched(case.name)
        fam, S = case.family, len(tab.str_slots)
        if fam == "empty_table":
            assert not tab.strings and tab.str_slots == [SLOT_EMPTY] * 2 and tab.pair_slots == [PAIR_EMPTY] * 2 and "tables-empty" in t
        elif fam == "tag_twin_absent":
            assert S == (2 if case.name.split("-")[3] == "2" else 4) and "miss-behind-tag-hit" in t
            assert not modelled(case.name, case.walkers[0])[0].bits[0] and modelled(case.name, case.walkers[0])[1].bits[0]
        elif fam == "tag_twins_present":
            want = "match-behind-two-tag-hits" if case.name == "triple-present" else "match-behind-tag-hit"
            assert S == (8 if case.name == "triple-present" else 4) and want in t and "occupied-behind-match" in t
            assert "two-tag-hits-then-miss" in t or case.name.endswith("-3")      # the absent third: the 10-letter namespace only
        elif fam == "tag_extremes":
            x = "0xFFFFF" if case.name == "tag-max" else "0"
            assert {"tag-%s-hit" % x, "tag-%s-twin" % x} <= t and S == 2
            assert tab.str_slots.count(0xFFFFF000) == (case.name == "tag-max") and tab.str_slots.count(0) == (case.name == "tag-zero")
        elif fam == "run_wrap":
            assert {"string-wrap", "match-behind-wrap", "miss-across-wrap", "miss-from-slot-0"} <= t
            assert tab.str_slots[S - 1] != SLOT_EMPTY and tab.str_slots[0] != SLOT_EMPTY
            assert sum(tab.slot0_of(s) == S - 1 for s in tab.strings) >= 2
        elif fam == "long_run":
            assert S == 4096 and len(tab.pair_slots) == 2048 and len(tab.strings) == 2048 and len(tab.pairs) == 1024
            assert sum(tab.slot0_of(s) == 4095 for s in tab.strings) == LONG_RUN
            assert {"run-60", "string-id-0", "string-id-2047", "cond-0", "cond-63", "cond-64", "cond-1023", "flag-word-15-bit-63",
                    "miss-across-wrap", "match-behind-wrap"} <= t
        elif fam == "roles_in_one_run":
            if case.name.startswith("roles"):
                assert {"role-filtered-path", "role-filtered-word"} <= t
                assert len({tab.slot0_of(s) for s in tab.strings}) == 1
                vs = modelled(case.name, case.walkers[0])
                assert not any(vs[0].bits) and not any(vs[1].bits) and all(vs[2].bits)
            else:
                assert tab.recs[0] >> 16 == (0 | 1 << 16 | 3 << 32)
        elif fam == "collision_behind_the_wrap":
            assert S == 4 and "collision" in t
            if case.name == "collision-path-only":
                assert {"role-filtered-other-bytes", "collision-behind-wrap"} <= t
            elif case.name.startswith("collision-wrap"):
                assert ("collision-behind-wrap" in t) == (case.name == "collision-wrap-xb")
            else:
                assert ("collision-behind-match" in t) == (case.name == "collision-both-ab") and ("match-behind-collision" in t) == (case.name == "collision-both-ba")
        elif fam == "pair_runs":
            P = len(tab.pair_slots)
            assert "pair-slots-%d" % P in t and "pair-hit" in t and tab.pair_slots[P - 1] != PAIR_EMPTY
            if P > 2:
                assert {"pair-wrap", "pair-hit-behind-wrap", "pair-miss-across-wrap", "pair-hit-behind-other", "pair-miss-behind-run"} <= t
                assert tab.pair_slots[0] != PAIR_EMPTY
        elif fam == "one_leaf":
            vs = modelled(case.name, case.walkers[0])
            assert [v.bits[0] for v in vs] == [True, False, False, False, False, False, True, True, False, False, True]
            assert {"leaf-resets-fid", "null-leaf-sets-fid", "leaf-sets-fid", "field-token-and-pair-from-one-leaf"} <= t and all(vs[10].bits)


_assert_properties()


# ---- expected verdicts: the oracle walker's matcher and the two tokenizer restatements, never the model ----

def condition_expression(cond):
    """the query of one (kind, field bytes, token bytes) condition, or None where a string is not text (the collision partner)"""
    kind, f, t = cond
    try:
        f, t = f.decode("utf-8"), t.decode("utf-8")
    except UnicodeDecodeError:
        return None
    c = {"Type": ("FIELD", "TOKEN", "FIELD_TOKEN")[kind], "Field": f, "Token": t}
    return {"ExpressionType": "CONDITION", "Condition": c}


def oracle_verdict(row: bytes, walker: str, expression) -> bool:
    if walker == "default":
        from oracle import walker_oracle as W
        return bool(W.matches_bloom_expression(row, expression))
    from tests import ngram_restatement as G, tokenizer_restatement as R
    return bool((R if walker == "separator" else G).row_verdict(row, spec_of(walker), expression))


def n_queries(case: Case) -> int:
    return len(case.conds) + len(case.composites)


FIELD_REGEX = 3                                # kKindFieldRegex
RX_COND = (FIELD_REGEX, b"rxf", b"^a")         # the regex instances' one FieldRegex condition, and the rows that give it a verdict
RX_ROWS = (b'{"rxf":"abc"}', b'{"rxf":"cba","k":"abc"}')
RX_REPLACED = 1022                             # in a table of 1 024 conditions it takes this one's place


def with_regex(case: Case) -> Case:
    """the case as bsg_match_rows_lookup_regex runs it: RX_COND behind the table (in a full table instead of condition 1 022, which no
    composite names: both tables keep their slot counts), RX_ROWS behind the rows.  The blob then lies behind lanes whose offset
    depends on this case's table sizes."""
    conds = list(case.conds)
    if len(conds) == MAX_CONDS:
        conds[RX_REPLACED] = RX_COND
        was, now = Table(case.conds), Table([c for c in conds if c[0] != FIELD_REGEX])
        assert (len(now.str_slots), len(now.pair_slots)) == (len(was.str_slots), len(was.pair_slots))
    else:
        conds.append(RX_COND)
    assert all(b"rxf" not in r for r in case.rows) and RX_REPLACED not in [x for k in case.composites for x in _terms(k)]
    return case._replace(name=case.name + "+regex", conds=tuple(conds), rows=case.rows + RX_ROWS)


def _terms(comp):
    if isinstance(comp, int):
        return [comp]
    return [] if comp is None else [t for k in comp[1:] for t in _terms(k)]


def expected(name: str, walker: str) -> np.ndarray:
    return expected_of(CASES[name], walker)


@functools.lru_cache(maxsize=None)
def expected_of(case: Case, walker: str) -> np.ndarray:
    """bool [n_queries][n_rows]: query c < n_conds is TERM c, the composites follow.  A condition whose string is not text occurs in
    no row's bytes (asserted), so it holds on none; the regex condition's verdict is tests/tokenizer_restatement.py's (Python re on the
    leaves at or under the field); a composite's value follows from its conditions' by And / Or."""
    out = np.zeros((n_queries(case), len(case.rows)), dtype=bool)
    for c, cond in enumerate(case.conds):
        if cond[0] == FIELD_REGEX:
            from tests import tokenizer_restatement as R
            rx = {"ExpressionType": "CONDITION", "Condition": {"Field": cond[1].decode(), "Pattern": cond[2].decode()}}
            out[c] = [R.row_verdict(r, R.SPECS["punct_lower"], None, rx) for r in case.rows]
            assert list(np.flatnonzero(out[c])) == [len(case.rows) - len(RX_ROWS)]
            continue
        e = condition_expression(cond)
        if e is None:
            assert all((cond[1] or cond[2]) not in r for r in case.rows)
            continue
        out[c] = [oracle_verdict(r, walker, e) for r in case.rows]
    for k, comp in enumerate(case.composites):
        out[len(case.conds) + k] = [comp_value(comp, out[: len(case.conds), r]) for r in range(len(case.rows))]
    out.setflags(write=False)
    return out


def differs(name: str, rule) -> bool:
    """does the rule change a verdict, a handed-back list or read a record no string has, on some row of the case?"""
    return any(modelled(name, w, rule) != modelled(name, w) and
               [v[:3] for v in modelled(name, w, rule)] != [v[:3] for v in modelled(name, w)] for w in CASES[name].walkers)


def first_broken(rule):
    return next((n for n in CASES if differs(n, rule)), None)


# rule -> the first case of the table (in its order) on which the rule changes a verdict, a handed-back list, or reads a record no
# string has; tests/test_lookup_shapes.py computes it again.  The two role rules differ from the rule as written only where the hash
# words are equal and the bytes are not: a key that is a word-only string's collision partner.
WRONG_RULE_BREAKS = {
    "stop at the first tag hit": "twins-present-ab",
    "take a tag hit as a match": "twin-absent-token-2",
    "no wrap in the string table": "twins-present-ab-3",
    "no wrap in the pair table": "pair-runs-4",
    "stop at the table's end instead of at the empty slot": "tag-max",
    "skip the role test": "collision-wrap-xb",
    "fingerprint before role": "collision-wrap-xb",
    "break behind a match": "collision-both-ab",
    "leaf_fid not reset at a leaf request": "one-leaf",
    "leaf_fid reset at a field request only": "one-leaf",
    "pair key with the ids swapped": "run-wrap-4096",
    "flag word index c >> 5": "run-wrap-4096",
}
