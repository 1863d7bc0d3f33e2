"""The distinct-entry tables at their edges, exactly.  Every case of tests/table_shapes.py puts entries PLACED by their base hashes —
a probe chain of exactly kMaxProbe, a cluster that wraps the table end, a table without an empty slot, a partition whose run is a
fraction of a slot, more than kPartThreads children, an LDS partition of exactly kPartFill entries ... — through set_insert2,
k_ingest_add, the rehash of grow_overflowed, both file-level union routes at seven partitionings, k_table_compact / merge_parents over
a context of two entries, and the walkers' dedup cache.  The reference is a Python set: counts are len(set), bitsets are the oracle's
build of the sorted set, status is 0 unless a murmur collision pair meets, and stats.table_grows is the number the occupancy model
forces (tests/test_table_shapes.py proves on the CPU that the table reaches the edges and that the numbers hold in every insertion
order): no case asserts a bound only."""
import numpy as np
import pytest

from bloomsearch_amd import ingest as I
from bloomsearch_amd.gpu import Context
from oracle import oracle as O
from tests import helpers as H
from tests import table_shapes as T

pytestmark = pytest.mark.gpu

FPR = 0.001
TRUSTED = 1                  # BSG_INGEST_TRUSTED_JSON
NO_PARENT = 0xFFFFFFFF
FLAGS = {"rows-validated": 0, "rows-trusted": TRUSTED}

_built = {}


def oracle_filter(entries):
    """O.build_sized of a set, once per distinct set of the session"""
    k = tuple(sorted(entries))
    if k not in _built:
        _built[k] = O.build_sized(list(k), FPR)
    return _built[k]


class Result:
    def __init__(self, counts, status, desc, words, stats):
        self.counts, self.status, self.desc, self.words, self.stats = counts, status, desc, words, stats

    def filter_words(self, index, kind):
        d = self.desc[index * 3 + kind]
        return self.words[int(d["word_off"]): int(d["word_off"]) + (int(d["m"]) + 63) // 64]


def hints_of(case):
    hints = np.zeros(len(case.children) * 3, dtype=np.uint32)
    for i, c in enumerate(case.children):
        hints[i * 3 + case.kind] = c.hint
    return hints


def parents_of(case):
    return [NO_PARENT if c.parent is None else c.parent for c in case.children] if case.n_parents else None


def finish(ctx, ing, case, build=True):
    counts, status = ctx.ingest_finish(ing, len(case.children) + case.n_parents)
    desc = words = None
    if build:
        desc, n_words = I.plan_desc(counts, FPR)
        words = ctx.ingest_build(ing, desc, n_words)
    return Result(counts, status, desc, words, ctx.ingest_stats(ing))


def run_add(ctx, case, build=True):
    """every batch in one bsg_ingest_add_entries call (k_ingest_add), each entry case.repeat times in a row: a wave's lanes on one slot"""
    ing = ctx.ingest_open(len(case.children), parents_of(case), case.n_parents, hints_of(case))
    try:
        for b in range(max(len(c.batches) for c in case.children)):
            entries, sets = [], []
            for i, c in enumerate(case.children):
                if b < len(c.batches):
                    entries += [e for e in c.batches[b] for _ in range(case.repeat)]
                    sets += [i] * (len(c.batches[b]) * case.repeat)
            if entries:
                ctx.ingest_add_entries(ing, entries, sets, [case.kind] * len(entries))
        return finish(ctx, ing, case, build)
    finally:
        ctx.ingest_free(ing)


def run_rows(ctx, case, flags):
    """one bsg_ingest_rows call: row {"k":"<word>"} per entry (the walkers' set_insert2: the token and its k::<word> per lane)"""
    row_sets = [[T.row_of(e, case.kind) for e in c.batches[0] for _ in range(case.repeat)] for c in case.children]
    assert all(len(c.batches) == 1 for c in case.children)
    res = I.device_ingest(ctx, row_sets, FPR, parent_of_set=parents_of(case), n_parents=case.n_parents, slots_hint=hints_of(case), flags=flags)
    assert len(res.fallback_rows) == 0
    return res


def run_stream(ctx, case):
    """bsg_ingest_append_rows: one append per batch (group stream), or the two sets' rows alternating in one append (group cache)"""
    with I.IngestStream.open(ctx, len(case.children), parents_of(case), case.n_parents, slots_hint=hints_of(case), flags=TRUSTED) as st:
        if case.group == "cache":
            rows, sor = T.cache_rows(case)
            assert len(st.append(rows, sor, finish_fallback=False)) == 0
        else:
            for b in range(max(len(c.batches) for c in case.children)):
                rows = [(T.row_of(e, case.kind), i) for i, c in enumerate(case.children) if b < len(c.batches) for e in c.batches[b]]
                assert len(st.append([r for r, _ in rows], [i for _, i in rows], finish_fallback=False)) == 0
                if case.group == "stream" and b == 0:
                    assert st.stats().table_grows == 0                     # the wrapping cluster is in place, nothing has grown yet
        return finish(ctx, st.id, case)


def run(ctx, case, route):
    how = T.insertion(case, route)
    if how == "add":
        return run_add(ctx, case)
    if how == "stream":
        return run_stream(ctx, case)
    return run_rows(ctx, case, FLAGS.get(route, TRUSTED))


def check_against_the_sets(case, route, res):
    """counts, status and bitsets of every table of every set and parent against the Python sets"""
    how = T.insertion(case, route)
    per_set = [[set(e for b in T.table_batches(case, c, kind, how) for e in b) for kind in range(3)] for c in case.children]
    per_parent = [[set().union(*[s[kind] for s, c in zip(per_set, case.children) if c.parent == p]) for kind in range(3)]
                  for p in range(case.n_parents)]
    assert not res.status.any(), (case.name, route, res.status)
    for index, sets in enumerate(per_set + per_parent):
        for kind in range(3):
            assert int(res.counts[index, kind]) == len(sets[kind]), (case.name, route, index, kind, int(res.counts[index, kind]), len(sets[kind]))
            want = oracle_filter(sets[kind])
            d = res.desc[index * 3 + kind]
            assert (int(d["m"]), int(d["k"])) == (want.m, want.k), (case.name, route, index, kind)
            assert np.array_equal(res.filter_words(index, kind), want.words), (case.name, route, index, kind)


def check_grows(case, route, res):
    exact, lower = T.predicted_grows(case, route)
    assert exact is not None and exact == lower, (case.name, route)           # every case of the table forces its number
    print("table_grows %s / %s: predicted %d, observed %d" % (case.name, route, exact, res.stats.table_grows))
    assert res.stats.table_grows == exact, (case.name, route, res.stats.table_grows, exact, case.why)


class union_route:
    """bsg_set_lab keys 9 (union route) and 10 (partitioning) for the length of a with-block"""

    def __init__(self, ctx, route):
        self.ctx, self.values = ctx, T.ROUTES.get(route, (0, 0))

    def __enter__(self):
        self.ctx.set_lab(T.KEY_UNION_MODE, self.values[0])
        self.ctx.set_lab(T.KEY_UNION_COARSEN, self.values[1])

    def __exit__(self, *exc):
        self.ctx.set_lab(T.KEY_UNION_MODE, 0)
        self.ctx.set_lab(T.KEY_UNION_COARSEN, 0)


PLAIN = [n for n, c in T.CASES.items() if c.group not in ("collision", "parts")]


@pytest.mark.parametrize("name", PLAIN)
def test_placed_entries_give_exact_counts_bitsets_and_growths(ctx, name):
    case = T.CASES[name]
    first = None
    for route in case.routes:
        with union_route(ctx, route):
            res = run(ctx, case, route)
        check_grows(case, route, res)
        if first is None or T.insertion(case, route) != T.insertion(case, case.routes[0]):
            check_against_the_sets(case, route, res)
            first = first or res
        else:
            # the routes against each other: what the first one gave has been compared with the sets bit for bit
            assert np.array_equal(res.counts, first.counts) and np.array_equal(res.status, first.status), (name, route)
            assert np.array_equal(res.desc, first.desc) and np.array_equal(res.words, first.words), (name, route)


def test_collision_pair_split_over_two_children_flags_only_the_parent(ctx):
    case = T.CASES["collision-pair-split"]
    for route in case.routes:
        with union_route(ctx, route):
            res = run_add(ctx, case, build=False)
        assert [int(res.counts[i, T.KIND_TOKEN]) for i in (0, 1)] == [1, 1], route
        assert list(res.status) == [0, 0, 2], (route, res.status)
        check_grows(case, route, res)


def test_parents_merged_over_two_parts_equal_one_device_and_the_sets(ctx):
    """bsg_set_lab key 8 = 1 cuts the call over the context's two entries (behind set 4: table_shapes.parts_cut): part 1's partial
    parents travel as dense lists of 1, 63, 64, 65 and 257 entries (k_table_compact) and k_ingest_union folds them, duplicates included"""
    case = T.CASES["two-parts"]
    with Context(H.device_ids(2)) as two:
        two.set_lab(T.KEY_SHARD_MIN_ROW_BYTES, 1)
        before = two.device_calls().copy()
        got = run_rows(two, case, TRUSTED)
        assert (two.device_calls() - before).min() >= 1                       # both entries of the context walked a part
    one = run_rows(ctx, case, TRUSTED)
    check_against_the_sets(case, "rows-trusted", got)
    assert np.array_equal(got.counts, one.counts) and np.array_equal(got.status, one.status) and np.array_equal(got.words, one.words)
    check_grows(case, "rows-trusted", got)
