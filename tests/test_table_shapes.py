"""tests/table_shapes.py kept honest, on the CPU: the restated placement functions against values computed another way from the
oracle's base hashes, the vectorised hash against the oracle's, every case's stated property in the occupancy model, the forced growth
numbers against insertions in random orders, every named edge reached by a case (computed from the table), the scan model against the
exact union at every partition count a case runs under, and deliberately wrong scan rules each of which must change some case's result
— or be listed as equivalent, with the reason, and then be equivalent on random tables too."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import table_shapes as T

CASES = T.CASES


def entries_of(case):
    return [e for c in case.children for b in c.batches for e in b]


def sample_entries():
    out = [bytes(w) for w in T.words("zz", 0, 64)] + [T.FT_PREFIX + bytes(w) for w in T.words("zy", 5, 64)]
    return out + [b"k", b"x" * 15, b"a longer entry that spans two murmur blocks"] + list(T.collision_pair())


# ---- the restatement ----

def test_constants_are_read_from_the_sources():
    assert set(T.K) == {"kMaxProbe", "kPartSlots", "kPartFill", "kPartTarget", "kPartThreads", "kPartProbes", "kPartAhead", "BSG_INGEST_CACHE_SETS"}
    assert all(v > 0 for v in T.K.values())               # (a changed constant moves the cases with it; a missing one fails the import)
    assert T.PART_FILL == T.PART_SLOTS * 3 // 4 and T.PART_SLOTS & (T.PART_SLOTS - 1) == 0
    assert [T.pow2_at_least(n) for n in (0, 1, 64, 65, 256, 257, 4096)] == [64, 64, 64, 128, 256, 512, 4096]


def test_placement_functions_agree_with_the_bits_of_the_oracles_hashes():
    """the same quantities from the binary expansion of h1 and h2 (bit 63 first), not from shifts and masks"""
    for e in sample_entries():
        h = O.base_hashes(e)
        b1, b2 = format(h[1], "064b"), format(h[2], "064b")
        key_bits = b1[64 - 52: 64 - 20]                     # bits 51 .. 20 of h1
        assert T.key(h) == int(key_bits, 2)
        for cap in (64, 256, 1024, 4096):
            assert T.home(h, cap) == int(key_bits[: cap.bit_length() - 1], 2)
        for lg in (1, 2, 6, 8, 10):
            assert T.partition(h, lg) == int(key_bits[:lg], 2)
        assert T.partition(h, 0) == 0
        assert T.lds_slot(h) == int(b2[64 - 28: 64 - 17], 2)                        # bits 27 .. 17 of h2
        assert T.cache_set(h) == (int(b1[64 - 24: 64 - 8], 2) * T.CACHE_SETS) // 65536 < T.CACHE_SETS


def test_vectorised_hash_equals_the_oracles():
    for prefix in (b"", T.FT_PREFIX, b"abcd"):
        w = T.words("qz", 123456, 200)
        blob = np.concatenate([np.broadcast_to(np.frombuffer(prefix, dtype=np.uint8), (len(w), len(prefix))), w], axis=1)
        hs = T.base_hashes_np(blob)
        for j in range(len(w)):
            assert tuple(int(h[j]) for h in hs) == O.base_hashes(blob[j].tobytes())
    assert len({bytes(x) for x in T.words("ab", 0, 26 ** 2 + 5)}) == 26 ** 2 + 5


def test_place_asserts_what_it_was_asked_and_fails_loudly():
    got = T.place("zx", 5, top=(6, 17), lds=None, cache=None)
    assert len(got) == 5 and all(T.home(T.hashes(e), 64) == 17 for e in got)
    got = T.place("zx", 3, T.KIND_FT, cache=7)
    assert all(e.startswith(T.FT_PREFIX) and T.cache_set(T.hashes(e)) == 7 for e in got)
    budget = T.SEARCH_BUDGET
    try:
        T.SEARCH_BUDGET = T.SEARCH_BATCH
        with pytest.raises(LookupError):
            T.place("zw", 3, top=(30, 12345))               # three entries sharing 30 key bits: not within one batch
    finally:
        T.SEARCH_BUDGET = budget


# ---- the occupancy model and the forced numbers ----

def advances(entries, cap, order):
    """the most advances of any entry when the distinct entries are inserted in this order, or None where one exceeds kMaxProbe"""
    slots, worst = [None] * cap, 0
    for j in order:
        s, n = T.home(T.hashes(entries[j]), cap), 0
        while slots[s] is not None:
            s, n = (s + 1) & (cap - 1), n + 1
            if n > T.MAX_PROBE:
                return None
        slots[s] = entries[j]
        worst = max(worst, n)
    return worst


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.group in ("insert", "stream")])
def test_forced_growths_hold_in_random_insertion_orders(name):
    """bound() and must_overflow() against plain insertions: whatever the order, the table grows exactly as often as forced_growths says"""
    case = CASES[name]
    entries = sorted(set(entries_of(case)))
    cap0 = T.table_cap(case, case.children[0], case.kind, "add")
    want = T.forced_growths(entries, cap0)
    assert want is not None, "the case's growth count depends on the order"
    rng = np.random.default_rng(7)
    orders = [np.arange(len(entries)), np.arange(len(entries))[::-1]] + [rng.permutation(len(entries)) for _ in range(6)]
    # ... and the adversarial one: the entries of the lowest home last
    homes = T.homes_of(entries, cap0 * T.GROWTH ** want)
    orders.append(np.argsort([-(h - min(homes)) for h in homes], kind="stable"))
    for order in orders:
        cap, grown = cap0, 0
        while advances(entries, cap, order) is None:
            cap, grown = cap * T.GROWTH, grown + 1
        assert grown == want, (name, grown, want)
        assert advances(entries, cap, order) <= T.bound(T.homes_of(entries, cap), cap) <= T.MAX_PROBE


def test_a_98_cluster_spread_evenly_would_depend_on_the_order():
    """why cluster() splits 2 + 96: 98 entries over four adjacent homes, none empty, form one run of 98 slots — forced_growths refuses"""
    es = sum((T.place("zv", n, top=(10, 0x5A << 2 | q)) for q, n in enumerate((25, 25, 24, 24))), ())
    assert T.forced_growths(es, 256) is None
    homes = T.homes_of(es, 1024)
    assert advances(es, 1024, np.argsort(homes, kind="stable")) is not None                      # lowest home first: fits
    assert advances(es, 1024, np.argsort([-h for h in homes], kind="stable")) is None             # lowest home last: 97 advances


EXPECTED_GROWS = {"same-home-96": 0, "same-home-97": 0, "same-home-98": 1, "same-home-98-top-10-bits": 2, "last-home-2": 0, "last-home-97": 0,
                  "last-home-98": 1, "full-64-of-64": 0, "full-64-then-one-more": 1, "same-home-97-x64": 0, "same-home-98-x64": 1,
                  "full-64-of-64-x64": 0, "ft-same-home-97": 0, "ft-same-home-98": 1, "ft-last-home-98": 1, "grow-across-appends": 1,
                  "lds-fill-%d" % T.PART_FILL: 0, "lds-fill-%d" % (T.PART_FILL + 1): 1, "lds-chain-%d" % T.PART_PROBES: 0,
                  "lds-chain-%d" % (T.PART_PROBES + 1): 1}


def test_every_route_of_every_case_has_a_forced_number():
    """the numbers the cases were made for, and exact predictions (not bounds) everywhere"""
    for name, case in CASES.items():
        for route in case.routes:
            exact, lower = T.predicted_grows(case, route)
            assert exact is not None and exact == lower, (name, route)
            if name in EXPECTED_GROWS:
                assert exact == EXPECTED_GROWS[name], (name, route, exact)
            elif name == "coarse-start-retries":
                assert exact == (1 if route == "coarse-then-retry" else 0), (name, route, exact)
            elif case.group in ("union", "many", "collision", "cache", "parts"):
                assert exact == 0, (name, route, exact)
    assert set(EXPECTED_GROWS) <= set(CASES)


def test_every_case_states_its_property():
    for name, case in CASES.items():
        assert case.why and all(r in (T.INSERT_ROUTES if case.group == "insert" else T.ROUTES) or r.startswith("rows") for r in case.routes)
        for c in case.children:
            for b in c.batches:
                assert len(set(b)) == len(b), name
        if case.group == "collision":
            a, b = (c.batches[0][0] for c in case.children)
            assert a != b and O.base_hashes(a) == O.base_hashes(b)
            continue
        # printable lower-case words under 16 bytes: the walker emits them unchanged
        for e in entries_of(case):
            assert len(e) < 16 and T.word_of(e, case.kind).isalpha() and T.word_of(e, case.kind).islower(), (name, e)
            assert e.startswith(T.FT_PREFIX) == (case.kind == T.KIND_FT)
    c = CASES["same-home-97"]
    cap = 256
    homes = T.homes_of(entries_of(c), cap)
    assert len(set(homes)) == 1 and T.bound(homes, cap) == T.MAX_PROBE
    occ = T.occupied(T.homes_of(entries_of(CASES["last-home-97"]), cap), cap)
    assert list(np.flatnonzero(occ)) == list(range(96)) + [255]                                  # "the cluster occupies cap - 1, 0, 1, ..."
    occ = T.occupied(T.homes_of(entries_of(CASES["last-home-98"]), 1024), 1024)
    assert list(np.flatnonzero(occ)) == list(range(95)) + [1020, 1021, 1023]                     # after the growth: 2, a gap, 96 that wrap
    full = CASES["full-64-then-one-more"].children[0]
    assert T.occupied(T.homes_of(full.batches[0], 64), 64).all() and len(full.batches[1]) == 1
    kid = CASES["child-full"].children[0]
    assert T.occupied(T.homes_of(kid.batches[0], 64), 64).all()
    # child-wraps: the wrapped cluster sits on partition 0's and 1's home slots, whose own entries lie behind it
    slots = T.child_tables(CASES["child-wraps"], 0)[0]
    displaced = [e for s, e in enumerate(slots) if e is not None and T.home(T.hashes(e), 64) in (0, 1) and s != T.home(T.hashes(e), 64)]
    assert slots[63] is not None and slots[0] is not None and T.home(T.hashes(slots[0]), 64) == 63 and len(displaced) == 9
    # run-97: in the 256-slot child the run is followed by an empty slot and crosses 97 / (256 / 1024) partitions' runs
    slots = T.child_tables(CASES["run-97-over-fine-partitions"], 0)[0]
    assert all(slots[0x21 + j] is not None for j in range(97)) and slots[0x21 + 97] is None and slots[0x20] is None
    for n in (T.PART_FILL, T.PART_FILL + 1):
        case = CASES["lds-fill-%d" % n]
        es = entries_of(case)
        assert len(es) == len(set(es)) == n and T.default_log2p(n) == 1
        assert all(T.partition(T.hashes(e), 1) == 0 for e in es) and len({T.lds_slot(T.hashes(e)) for e in es}) == n
        assert all(T.table_cap(case, c, case.kind, "add") == 4096 for c in case.children)
    for n in (T.PART_PROBES, T.PART_PROBES + 1):
        es = sorted(set(entries_of(CASES["lds-chain-%d" % n])))
        assert len(es) == n and len({T.lds_slot(T.hashes(e)) for e in es}) == 1 and T.default_log2p(2 * n) == 0
        assert max(np.bincount([T.partition(T.hashes(e), 2) for e in es])) <= 13
    for name in ("cache-3-shared", "cache-4-shared", "cache-4-overlap"):
        case = CASES[name]
        assert len({T.cache_set(T.hashes(e)) for e in entries_of(case)}) == 1 and len(set(entries_of(case))) > 2
        rows, sor = T.cache_rows(case)
        assert sor[:4] == [0, 1, 0, 1] and len(rows) <= 2 * 160 and set(T.child_sets(case)[0]) & set(T.child_sets(case)[1])
        for s in (0, 1):
            assert {r for r, x in zip(rows, sor) if x == s} == {T.row_of(e, case.kind) for e in case.children[s].batches[0]}
    parts = CASES["two-parts"]
    assert T.parts_cut(parts) == [0, len(T.PART_COUNTS), 2 * len(T.PART_COUNTS)]
    second = T.child_sets(parts)[len(T.PART_COUNTS):]
    first = T.child_sets(parts)[:len(T.PART_COUNTS)]
    assert tuple(len(s) for s in second) == T.PART_COUNTS
    assert [len(a & b) for a, b in zip(first, second)] == [n // 2 for n in T.PART_COUNTS]


def test_route_names_tell_the_partition_count():
    """the counts of every case that runs under all routes sum to kPartTarget at most per parent table: the default is one partition"""
    want = {"default": 0, "2-partitions": 1, "64-partitions": 6, "256-partitions": 8, "1024-partitions": 10, "coarse-then-retry": 0}
    for name, case in CASES.items():
        if case.routes != T.ALL_ROUTES:
            continue
        how = T.insertion(case, "default")
        for p in range(case.n_parents):
            for kind in range(3):
                total = sum(len(set(e for b in T.table_batches(case, c, kind, how) for e in b)) for c in case.children if c.parent == p)
                assert total <= T.PART_TARGET, name
                for route, lg in want.items():
                    assert T.route_log2p(total, T.ROUTES[route][1]) == lg
        assert T.scan_log2ps(case) == [0, 1, 6, 8, 10]


# ---- every named edge is reached ----

def _placed(case, child=0):
    c = case.children[child]
    return c, T.table_cap(case, c, case.kind, "add"), [e for b in c.batches for e in b]


def edge_chain_of_exactly_max_probe(case):
    c, cap, es = _placed(case)
    return case.group == "insert" and T.forced_growths(es, cap) == 0 and T.bound(T.homes_of(es, cap), cap) == T.MAX_PROBE


def edge_one_home_over_the_bound(case):
    c, cap, es = _placed(case)
    return case.group == "insert" and max(np.bincount(T.homes_of(es, cap))) == T.MAX_PROBE + 2


def edge_cluster_wraps(case):
    c, cap, es = _placed(case)
    homes = T.homes_of(es, cap)
    occ = T.occupied(homes, cap) if len(es) <= cap else None
    return case.group == "insert" and occ is not None and homes.count(cap - 1) >= 2 and occ[cap - 1] and occ[0]


def edge_child_without_an_empty_slot(case):
    return case.group in T.SCAN_GROUPS and any(t is not None and all(s is not None for s in t) for t in T.child_tables(case, 0))


def edge_rehash_reads_a_full_table(case):
    c, cap, es = _placed(case)
    return len(c.batches) == 2 and len(c.batches[0]) == cap and T.batch_growths([list(b) for b in c.batches], cap) == 1


def edge_run_is_a_fraction_of_a_slot(case):
    return case.group in T.SCAN_GROUPS and any((1 << lg) > len(t) for lg in T.scan_log2ps(case) for t in T.child_tables(case, 0))


def edge_spill_crosses_many_partitions(case):
    if case.group not in T.SCAN_GROUPS:
        return False
    for t in T.child_tables(case, 0):
        if len(t) > 256:
            continue                          # (the placed runs are in the small children)
        for lg in T.scan_log2ps(case):
            away = [abs(T.partition(T.hashes(e), lg) - ((s << lg) // len(t))) for s, e in enumerate(t) if e is not None]
            if away and max(away) >= 16 and (1 << lg) <= len(t) * 16:
                return True
    return False


EDGES = {
    "a probe chain of exactly kMaxProbe": edge_chain_of_exactly_max_probe,
    "one home holds kMaxProbe + 2": edge_one_home_over_the_bound,
    "two growths in a row": lambda case: case.group == "insert" and T.forced_growths(_placed(case)[2], _placed(case)[1]) == 2,
    "a cluster wraps the table end": edge_cluster_wraps,
    "a wrapping cluster in the field::token table (entry B of set_insert2)": lambda case: case.kind == T.KIND_FT and edge_cluster_wraps(case),
    "a child table without an empty slot": edge_child_without_an_empty_slot,
    "a rehash reads a table without an empty slot": edge_rehash_reads_a_full_table,
    "every entry 64 times in one call, at the bound": lambda case: case.repeat == 64 and T.forced_growths(_placed(case)[2], _placed(case)[1]) == 1,
    "a later append overflows a wrapping cluster": lambda case: case.group == "stream" and T.batch_growths([list(b) for b in _placed(case)[0].batches], 256) == 1
    and T.occupied(T.homes_of(_placed(case)[0].batches[0], 256), 256)[[255, 0]].all(),
    "a partition's run is a fraction of a slot": edge_run_is_a_fraction_of_a_slot,
    "a probe spill crosses sixteen partitions and more": edge_spill_crosses_many_partitions,
    "children of three capacities under one parent": lambda case: case.group == "union" and len({len(t) for t in T.child_tables(case, 0)}) >= 3,
    "an empty child and a child of one entry": lambda case: case.group == "union" and {0, 1} <= {len(s) for s in T.child_sets(case)},
    "a parent with no child": lambda case: any(all(c.parent != p for c in case.children) for p in range(case.n_parents)),
    "more than kPartThreads children": lambda case: T.PART_THREADS < len(case.children) <= 2 * T.PART_THREADS,
    "more than 2 kPartThreads children": lambda case: len(case.children) > 2 * T.PART_THREADS,
    "an LDS partition of exactly kPartFill": lambda case: case.group == "fill" and len(set(entries_of(case))) == T.PART_FILL and T.union_retries(T.child_sets(case), 0) == 0,
    "an LDS partition of kPartFill + 1": lambda case: case.group == "fill" and len(set(entries_of(case))) == T.PART_FILL + 1 and T.union_retries(T.child_sets(case), 0) == 1,
    "an LDS chain of kPartProbes entries": lambda case: case.group == "probes" and len(set(entries_of(case))) == T.PART_PROBES and T.union_retries(T.child_sets(case), 0) == 0,
    "an LDS chain of kPartProbes + 1": lambda case: case.group == "probes" and len(set(entries_of(case))) == T.PART_PROBES + 1 and T.union_retries(T.child_sets(case), 0) == 1,
    "a collision pair that meets only in the parent": lambda case: case.group == "collision",
    "dense lists of 1, 63, 64, 65 and 257 entries": lambda case: case.group == "parts" and {1, 63, 64, 65, 257} <= {len(s) for s in T.child_sets(case)},
    "more words than ways in one dedup-cache set, shared by two sets": lambda case: case.group == "cache" and len(set(entries_of(case))) == 4,
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_every_named_edge_is_reached(edge):
    assert [name for name, case in CASES.items() if EDGES[edge](case)], edge


# ---- the scan model ----

SCAN_CASES = [n for n, c in CASES.items() if c.group in T.SCAN_GROUPS]


def union_of(case):
    return T.parent_sets(case)[0]


@pytest.mark.parametrize("name", SCAN_CASES)
def test_scan_rule_as_written_finds_exactly_the_union(name):
    case = CASES[name]
    tables = T.child_tables(case, 0)
    want = union_of(case)
    for lg in T.scan_log2ps(case):
        count, entries = T.scan_union(tables, lg)
        assert entries == want and count == len(want), (name, lg, count, len(want))


class NoChainPastTheEnd(T.ScanRule):
    name, chain_past_end = "no chain past the run's end", False


class NoWrap(T.ScanRule):
    name, wrap = "no wrap", False


class StopAtAGapInsideTheRun(T.ScanRule):
    name, gap_inside_stops = "a stop at the first gap inside the run", True


class NoKeyFilter(T.ScanRule):
    name, key_filter = "no key filter", False


class FloorEnd(T.ScanRule):
    name, ceil_end = "the run's end taken as floor", False


class LateGap(T.ScanRule):
    name, late_gap = "the gap test one slot later", True


WRONG_RULES = (NoChainPastTheEnd, NoWrap, StopAtAGapInsideTheRun, NoKeyFilter)
# Rules that differ in the text and not in any result, with the reason.  They are not dropped: the test below shows that no case AND no
# random table tells them from the rule as written.
EQUIVALENT_RULES = {
    FloorEnd: "with the end as floor a run of a fraction of a slot is empty ([h, h)), but `chain` starts true at the run's first slot, so "
              "slot h is looked at all the same, and the gap test `s + u + 1 >= e` holds from slot h on under either end; where the "
              "partitions are no more than the slots the two ends are the same integer",
    LateGap: "a gap AT the run's last slot is then not noticed, so the scan only goes on to the next gap: it looks at more slots, and "
             "the key filter drops what is not the partition's",
}


def differs(rule, name):
    case = CASES[name]
    tables = T.child_tables(case, 0)
    want = union_of(case)
    return any(T.scan_union(tables, lg, rule) != (len(want), want) for lg in T.scan_log2ps(case))


@pytest.mark.parametrize("rule", WRONG_RULES, ids=lambda r: r.name)
def test_every_wrong_scan_rule_changes_some_case(rule):
    small = [n for n in SCAN_CASES if CASES[n].group == "union"]
    assert [n for n in small if differs(rule, n)], rule.name


@pytest.mark.parametrize("rule", list(EQUIVALENT_RULES), ids=lambda r: r.name)
def test_equivalent_rules_are_equivalent(rule):
    assert EQUIVALENT_RULES[rule]
    for name in SCAN_CASES:
        if CASES[name].group == "union":
            assert not differs(rule, name), name
    # ... and on random and skewed tables of 64 to 256 slots at loads 0.2 to 1.0 under 1 to 1 024 partitions
    for trial, (tables, want) in enumerate(random_tables()):
        for lg in (0, 3, 6, 8, 10):
            assert T.scan_union(tables, lg, rule) == (len(want), want), (rule.name, trial, lg)


_random_tables = []


def random_tables():
    """[(three child tables, their union)], checked once against the rule as written"""
    if not _random_tables:
        rng = np.random.default_rng(11)
        pool = T.place("zu", 600) + T.cluster("zt", 60, 6, 63) + T.cluster("zs", 90, 8, 0x21)
        for trial in range(9):
            tables = []
            for _ in range(3):
                cap = int(rng.choice([64, 128, 256]))
                n = max(1, int(cap * rng.choice([0.2, 0.6, 0.9, 1.0])))
                skew = pool[600:] if trial % 3 == 0 else ()
                picks = [pool[j] for j in rng.choice(600, size=n, replace=False)]
                tables.append(T.fill((list(skew) + picks)[:n], cap))
            want = set(e for t in tables for e in t if e is not None)
            for lg in (0, 3, 6, 8, 10):
                assert T.scan_union(tables, lg) == (len(want), want), (trial, lg)
            _random_tables.append((tables, want))
    return _random_tables
