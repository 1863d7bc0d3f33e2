"""The distinct-entry tables of device ingest (csrc/ingest.hip.h) at the edges of their probing, growing and union code: the table of
cases tests/test_table_edges_gpu.py runs, entries PLACED where a case needs them, and plain models of what the tables and the file-level
union do with them.  tests/test_table_shapes.py keeps this file honest (the restated placement functions against values computed from the
oracle's base hashes, every case's stated property in the occupancy model, coverage of every named edge computed from the table, the scan
model against the exact union, and a list of deliberately wrong scan rules).  Test infrastructure only: no GPU, no call into the library.

Placement.  An entry's slot is a pure function of its base hashes (h0, h1, h2, h3) = (murmur(d), murmur(d || 0x01)):
    table key            (h1 >> 20) & 0xFFFFFFFF                        table_key
    home slot, 2^b slots the key's top b bits                            insert_begin
    partition, 2^L       the key's top L bits                            k_union_partitions
    LDS slot             (h2 >> 17) & (kPartSlots - 1)                   k_union_partitions
    dedup-cache set      (((h1 >> 8) & 0xFFFF) * kCacheSets) >> 16       cache_set
place() searches a namespace of 10-letter lower-case words (a two-letter tag, then a counter in base 26) for entries with the wanted
bits: the walker emits such a word unchanged as a token, and as "k::" + word from a row {"k":"<word>"}.  The search hashes whole
batches with a numpy MurmurHash3_x64_128 for inputs shorter than 16 bytes (tail only, no block loop); everything it returns is hashed
again with the oracle's base_hashes and every requested property is asserted on those.

What makes outcomes — not only results — predictable.  With linear probing the SET of occupied slots does not depend on the insertion
order, and an entry that ends j slots behind its home has advanced exactly j times (a lost claim looks at the same slot again, a
duplicate finds its twin).  So with E the last slot of the cluster an entry's home lies in, the entry advances at most E - home times
in ANY order (bound()); where that is <= kMaxProbe for every entry the table cannot overflow, and where one home holds
kMaxProbe + 2 entries (or the table more entries than slots) it must.  forced_growths() applies the two tests capacity by capacity
(x 4 per growth, grow_overflowed) and answers None where neither holds.  A cluster of 98 that shares the key's top b bits is therefore
made of 2 entries whose next two bits are 00 and 96 whose next two bits are 11: four times the capacity later the two groups are
separated by an empty slot and neither can overflow — 98 entries spread over four adjacent homes in any other way form one run of 98
slots, and the entry of the first home that arrives last advances 97 times: a second growth that depends on the order.

Not reachable at test size, and left out: the kSpinLimit path (a claimer context-switched out between its CAS and its stores), the
"still overflow after 12 growth rounds" error (about 100 entries sharing 30 key bits: not searchable), tables near 2^31 slots.  No
case is meant to hang or fault, and the library's constants are read here, never set.

Cost.  Generating every placement of the table (this module's import) takes 0.8 s on the development machine, one core; the
vectorised hash does about 4 M candidates a second, so neither the 1 537 pairwise different LDS slots nor the 49 entries that share 11
bits of h2 and two key bits needed thinning: every case asserts its forced number, none results only.  tests/test_table_shapes.py
runs in 6 s there, tests/test_build_shapes.py in 7 s.
"""
from __future__ import annotations

import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- constants, from the sources ----

def source_constant(rel_path: str, name: str, known: dict) -> int:
    """a `constexpr <type> NAME = <expression>;` of a source file, evaluated over the constants read before it (as
    build_shapes.source_constant; an integer division is allowed here: kPartFill = kPartSlots * 3 / 4)"""
    src = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", rel_path)).read()
    found = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
    if not found:
        raise LookupError("%s: no constexpr %s" % (rel_path, name))
    expr = re.sub(r"\b(\d+)(?:ull|ul|u)\b", r"\1", found.group(1), flags=re.I)
    if not re.fullmatch(r"[\w\s*+()</-]+", expr) or "//" in expr:
        raise LookupError("%s: %s = %s is not plain arithmetic" % (rel_path, name, expr))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(known)))


K = {}
for _name in ("kMaxProbe", "kPartSlots", "kPartFill", "kPartTarget", "kPartThreads", "kPartProbes", "kPartAhead"):
    K[_name] = source_constant("ingest.hip.h", _name, K)


def source_define(rel_path: str, name: str) -> int:
    src = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", rel_path)).read()
    found = re.search(r"#define\s+%s\s+(\d+)\s*$" % name, src, flags=re.M)
    if not found:
        raise LookupError("%s: no #define %s" % (rel_path, name))
    return int(found.group(1))


K["BSG_INGEST_CACHE_SETS"] = source_define("ingest.hip.h", "BSG_INGEST_CACHE_SETS")

MAX_PROBE = K["kMaxProbe"]
PART_SLOTS, PART_FILL, PART_TARGET = K["kPartSlots"], K["kPartFill"], K["kPartTarget"]
PART_THREADS, PART_PROBES, PART_AHEAD = K["kPartThreads"], K["kPartProbes"], K["kPartAhead"]
CACHE_SETS = K["BSG_INGEST_CACHE_SETS"]
MIN_CAP = 64                 # pow2_at_least (host/ingest_plan.hpp): a hint is rounded up to a power of two, 64 at least
GROWTH = 4                   # grown_slots (host/ingest_plan.hpp; grow_overflowed in ingest_api.inc): an overflowed table gets four times its slots
# capacities where the caller gives no hint (host/ingest_plan.hpp): oneshot_slots for ingest_rows_part (fields 256; tokens and
# field::tokens max(1024, 4 x rows)) and stream_slots for stream_add_sets (256 and 1024)
DEFAULT_FIELD_SLOTS, DEFAULT_TOKEN_SLOTS = 256, 1024
KIND_FIELD, KIND_TOKEN, KIND_FT = 0, 1, 2
KEY_SHARD_MIN_ROW_BYTES, KEY_UNION_MODE, KEY_UNION_COARSEN = 8, 9, 10     # bsg_set_lab keys
WORD_LEN = 10
FT_PREFIX = b"k::"
ROW_BYTES = len(b'{"k":""}') + WORD_LEN


def pow2_at_least(n: int) -> int:
    c = MIN_CAP
    while c < n:
        c <<= 1
    return c


# ---- placement functions of one entry, restated over Python integers ----

def key(h) -> int:
    return (h[1] >> 20) & 0xFFFFFFFF


def home(h, cap: int) -> int:
    b = cap.bit_length() - 1
    assert 1 << b == cap
    return key(h) >> (32 - b)


def partition(h, log2p: int) -> int:
    return key(h) >> (32 - log2p) if log2p else 0


def lds_slot(h) -> int:
    return (h[2] >> 17) & (PART_SLOTS - 1)


def cache_set(h) -> int:
    return ((((h[1] >> 8) & 0xFFFF) * CACHE_SETS) >> 16)


@functools.lru_cache(maxsize=None)
def hashes(entry: bytes):
    from oracle import oracle as O
    return O.base_hashes(entry)


# ---- a vectorised murmur3_x64_128 (seed 0) for inputs of fewer than 16 bytes ----

_C1, _C2 = np.uint64(0x87C37B91114253D5), np.uint64(0x4CF5AD432745937F)


def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _fmix(k):
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xFF51AFD7ED558CCD)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xC4CEB9FE1A85EC53)
    return k ^ (k >> np.uint64(33))


def _murmur_tail(lo, hi, n: int):
    """(h1, h2) of inputs of n < 16 bytes held little-endian in (lo, hi), bytes from n on zero"""
    assert 0 < n < 16
    h1 = _rotl(lo * _C1, 31) * _C2
    h2 = _rotl(hi * _C2, 33) * _C1 if n > 8 else np.zeros_like(lo)
    h1 = h1 ^ np.uint64(n)
    h2 = h2 ^ np.uint64(n)
    h1 = h1 + h2
    h2 = h2 + h1
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = h1 + h2
    return h1, h2 + h1


def base_hashes_np(blob: np.ndarray):
    """blob u8 [N][L], L <= 14 -> (h0, h1, h2, h3), each u64 [N]"""
    n, length = blob.shape
    assert length <= 14
    buf = np.zeros((n, 16), dtype=np.uint8)
    buf[:, :length] = blob
    w = buf.view("<u8")
    h0, h1 = _murmur_tail(w[:, 0], w[:, 1], length)
    buf[:, length] = 1
    h2, h3 = _murmur_tail(w[:, 0], w[:, 1], length + 1)
    return h0, h1, h2, h3


def words(tag: str, first: int, n: int) -> np.ndarray:
    """u8 [n][WORD_LEN]: the tag's two letters, then first .. first + n - 1 in base 26 (a .. z), most significant digit first"""
    assert len(tag) == 2 and tag.isalpha() and tag.islower()
    out = np.empty((n, WORD_LEN), dtype=np.uint8)
    out[:, 0], out[:, 1] = ord(tag[0]), ord(tag[1])
    v = np.arange(first, first + n, dtype=np.int64)
    for col in range(WORD_LEN - 1, 1, -1):
        out[:, col] = ord("a") + v % 26
        v = v // 26
    return out


SEARCH_BATCH = 1 << 16
SEARCH_BUDGET = 1 << 23                       # candidates per place() call


@functools.lru_cache(maxsize=None)
def place(tag: str, n: int, kind: int = KIND_TOKEN, top=None, lds=None, cache=None, distinct_lds: bool = False):
    """n entries of the tag's namespace, the first that fit in counter order.  kind: KIND_TOKEN — the words themselves; KIND_FT —
    "k::" + word.  top = (b, v): the key's top b bits are v; lds: the LDS slot; cache: the dedup-cache set; distinct_lds: pairwise
    different LDS slots.  Raises when SEARCH_BUDGET candidates did not hold n; never returns fewer."""
    prefix = np.frombuffer(FT_PREFIX if kind == KIND_FT else b"", dtype=np.uint8)
    found, slots_taken, first = [], set(), 0
    while len(found) < n:
        if first >= SEARCH_BUDGET:
            raise LookupError("place(%s): %d of %d entries within %d candidates" % (tag, len(found), n, SEARCH_BUDGET))
        w = words(tag, first, SEARCH_BATCH)
        blob = np.concatenate([np.broadcast_to(prefix, (len(w), len(prefix))), w], axis=1) if len(prefix) else w
        _, h1, h2, _ = base_hashes_np(blob)
        k32 = (h1 >> np.uint64(20)) & np.uint64(0xFFFFFFFF)
        ok = np.ones(len(w), dtype=bool)
        if top is not None:
            ok &= (k32 >> np.uint64(32 - top[0])) == np.uint64(top[1])
        slot = ((h2 >> np.uint64(17)) & np.uint64(PART_SLOTS - 1)).astype(np.int64)
        if lds is not None:
            ok &= slot == lds
        if cache is not None:
            ok &= ((((h1 >> np.uint64(8)) & np.uint64(0xFFFF)) * np.uint64(CACHE_SETS)) >> np.uint64(16)) == np.uint64(cache)
        for j in np.flatnonzero(ok):
            if distinct_lds:
                if int(slot[j]) in slots_taken:
                    continue
                slots_taken.add(int(slot[j]))
            found.append(blob[j].tobytes())
            if len(found) == n:
                break
        first += SEARCH_BATCH
    # every entry again, through the oracle's hash and the scalar restatements
    hs = [hashes(e) for e in found]
    assert len(set(found)) == n and all(e.isalpha() or kind == KIND_FT for e in found)
    assert all(len(e) < 16 and e[len(prefix):].isalpha() and e[len(prefix):].islower() for e in found)
    if top is not None:
        assert all(key(h) >> (32 - top[0]) == top[1] for h in hs), tag
    if lds is not None:
        assert all(lds_slot(h) == lds for h in hs), tag
    if cache is not None:
        assert all(cache_set(h) == cache for h in hs), tag
    if distinct_lds:
        assert len({lds_slot(h) for h in hs}) == n, tag
    return tuple(found)


def cluster(tag: str, n: int, bits: int, value: int, kind: int = KIND_TOKEN):
    """n entries whose keys share their top `bits` bits (= value): 2 whose next two bits are 00, n - 2 whose next two are 11 (see the
    module docstring) — in a table of 2^bits slots one home, in one of four times the slots two runs with an empty slot between them"""
    assert n >= 2
    out = place(tag, 2, kind, top=(bits + 2, value << 2)) + place(tag, n - 2, kind, top=(bits + 2, value << 2 | 3))
    hs = [hashes(e) for e in out]
    assert len({key(h) >> (32 - bits) for h in hs}) == 1 and len({key(h) >> (30 - bits) for h in hs}) == min(n - 1, 2)
    assert max(np.bincount(homes_of(out, GROWTH << bits))) == max(n - 2, 2)      # never n in one home after one growth
    return out


def homes_of(entries, cap: int):
    return [home(hashes(e), cap) for e in entries]


def companion(entry: bytes, kind: int) -> bytes:
    """the entry a row {"k":"<word>"} puts into the OTHER of the token and field::token tables"""
    return FT_PREFIX + entry if kind == KIND_TOKEN else entry[len(FT_PREFIX):]


def word_of(entry: bytes, kind: int) -> bytes:
    return entry if kind == KIND_TOKEN else entry[len(FT_PREFIX):]


def row_of(entry: bytes, kind: int) -> bytes:
    return b'{"k":"' + word_of(entry, kind) + b'"}'


# ---- occupancy model: linear probing into cap slots ----

def occupied(homes, cap: int):
    """bool [cap]: the slots n entries with these homes end in — the same for every insertion order"""
    occ = np.zeros(cap, dtype=bool)
    for g in homes:
        s = g
        for _ in range(cap):
            if not occ[s]:
                occ[s] = True
                break
            s = (s + 1) & (cap - 1)
    return occ


def fill(entries, cap: int):
    """[cap] of entry or None: the table after inserting the entries in this order (which entry sits where depends on the order; which
    slots are taken does not)"""
    slots = [None] * cap
    for e in entries:
        s = home(hashes(e), cap)
        for _ in range(cap):
            if slots[s] is None or slots[s] == e:
                slots[s] = e
                break
            s = (s + 1) & (cap - 1)
        else:
            raise AssertionError("no room")
    return slots


def bound(homes, cap: int) -> int:
    """the most advances any entry can make in any insertion order: last slot of its cluster - its home (cap - 1 in a full table)"""
    occ = occupied(homes, cap)
    if occ.all():
        return cap - 1
    worst = 0
    for g in set(homes):
        j = 0
        while occ[(g + j + 1) & (cap - 1)]:
            j += 1
        worst = max(worst, j)
    return worst


def must_overflow(homes, cap: int) -> bool:
    """more entries than slots, or kMaxProbe + 2 of one home: the last of them to settle has advanced more than kMaxProbe times"""
    return len(homes) > cap or (len(homes) > 0 and int(np.bincount(homes).max()) >= MAX_PROBE + 2)


def forced_growths(entries, cap: int, limit: int = 1 << 20):
    """growths the distinct entries force on a table of cap slots whatever the order — or None where the order decides"""
    entries = sorted(set(entries))
    grown = 0
    while cap <= limit:
        homes = homes_of(entries, cap)
        if must_overflow(homes, cap):
            cap *= GROWTH
            grown += 1
        elif bound(homes, cap) <= MAX_PROBE:
            return grown
        else:
            return None
    return None


# ---- scan model: k_union_partitions over the children's tables ----

class ScanRule:
    """The rule as written.  The hooks are where tests/test_table_shapes.py's wrong rules differ."""
    name = "as written"
    chain_past_end = True        # past the run keep looking while no gap has been seen from the run's last slot on
    wrap = True                  # slot indices wrap by & mask
    ceil_end = True              # the run ends at ceil((p + 1) cap / P)
    gap_inside_stops = False     # (wrong) the first empty slot ends the child, wherever it lies
    key_filter = True            # keep an entry only if its key belongs to the partition
    late_gap = False             # (equivalent) the gap test starts one slot behind the run's last


def scan_child(slots, p: int, log2p: int, rule=ScanRule):
    """the entries partition p of 2^log2p takes from one child table ([cap] of entry or None)"""
    cap = len(slots)
    s = (p * cap) >> log2p
    e = ((p + 1) * cap + ((1 << log2p) - 1 if rule.ceil_end else 0)) >> log2p
    found, scanned = [], 0
    while True:
        chain = True
        for u in range(PART_AHEAD):
            at = s + u
            entry = slots[at & (cap - 1)] if (rule.wrap or at < cap) else None
            look = entry is not None and (at < e or (chain and rule.chain_past_end))
            if rule.gap_inside_stops and not chain:
                look = False
            if look and (not rule.key_filter or partition(hashes(entry), log2p) == p):
                found.append(entry)
            if entry is None and (rule.gap_inside_stops or at + (0 if rule.late_gap else 1) >= e):
                chain = False
        scanned += PART_AHEAD
        s += PART_AHEAD
        if scanned > cap:                       # a table without an empty slot: one lap
            break
        if (s >= e or rule.gap_inside_stops) and not chain:
            break
        if not rule.chain_past_end and s >= e:
            break
    return found


def scan_union(tables, log2p: int, rule=ScanRule):
    """(count, entries): what the partitions' workgroups add to the parent's counter in all — every partition its distinct finds —
    and the entries they write"""
    count, entries = 0, set()
    tables = list(dict.fromkeys(tuple(t) for t in tables))      # (a set union: a table seen twice adds nothing)
    for p in range(1 << log2p):
        mine = set()
        for slots in tables:
            mine.update(scan_child(slots, p, log2p, rule))
        count += len(mine)
        entries |= mine
    return count, entries


def default_log2p(total: int) -> int:
    """union_partitioned: the coarsest partitioning with at most kPartTarget child entries (duplicates included) per partition"""
    lg = 0
    while (total >> lg) > PART_TARGET and lg < 24:
        lg += 1
    return lg


def route_log2p(total: int, coarsen: int) -> int:
    lg = default_log2p(total)
    return lg - min(lg, coarsen) if coarsen < 32 else min(lg + coarsen - 32, 24)


def lds_fits(entries):
    """does one partition's LDS table take these distinct entries?  True / False where every order agrees, None where it does not"""
    if len(entries) > PART_FILL:
        return False
    slots = [lds_slot(hashes(e)) for e in entries]
    if slots and int(np.bincount(slots).max()) > PART_PROBES:      # the last of PART_PROBES + 1 of one slot needs PART_PROBES advances
        return False
    return True if bound(slots, PART_SLOTS) < PART_PROBES else None


def union_retries(child_sets, coarsen: int):
    """4-x-finer retries of the partitioned union over these children's distinct entries (None: the order decides; 4: it gives up and
    takes the global tables, which this table never reaches)"""
    total = sum(len(c) for c in child_sets)
    everything = set().union(*child_sets) if child_sets else set()
    lg, tries = route_log2p(total, coarsen), 0
    while tries < 4:
        parts = {}
        for e in everything:
            parts.setdefault(partition(hashes(e), lg), []).append(e)
        verdicts = [lds_fits(es) for es in parts.values()]
        if any(v is False for v in verdicts):
            lg, tries = min(lg + 2, 26), tries + 1
        elif all(v is True for v in verdicts):
            return tries
        else:
            return None
    return tries


# ---- the table ----

# hint: what the caller asks for the PLACED table (kind of the case) of this set; the other two keep their defaults.  parent: index or
# None.  batches: one tuple of entries per call (bsg_ingest_add_entries) or per append; a rows route with one batch is one call.
Child = namedtuple("Child", "hint parent batches")
# group: insert / stream / union / many / fill / probes / collision / parts / cache.  kind: the placed table.  routes: names of ROUTES
# (union groups) or of INSERT_ROUTES.  repeat: every entry is handed in this many times per call.  why: the one-line argument for the
# numbers the case forces.
Case = namedtuple("Case", "name group kind children n_parents routes repeat why")

INSERT_ROUTES = ("add", "rows-validated", "rows-trusted")
# name -> (lab key 9, lab key 10).  The partition counts named hold where the children's counts sum to kPartTarget at most (the default
# is then ONE partition): tests/test_table_shapes.py asserts that of every case these run under.
ROUTES = {"default": (0, 0), "2-partitions": (0, 32 + 1), "64-partitions": (0, 32 + 6), "256-partitions": (0, 32 + 8),
          "1024-partitions": (0, 32 + 10), "global-tables": (1, 0), "coarse-then-retry": (0, 4)}
ALL_ROUTES = tuple(ROUTES)


def child_sets(case: Case):
    return [set(e for b in c.batches for e in b) for c in case.children]


def parent_sets(case: Case):
    sets = child_sets(case)
    return [set().union(*[s for s, c in zip(sets, case.children) if c.parent == p]) for p in range(case.n_parents)]


def insertion(case: Case, route: str) -> str:
    """how the entries reach the device: "add" (bsg_ingest_add_entries into an opened ingest), "rows" (one bsg_ingest_rows call) or
    "stream" (bsg_ingest_append_rows, one append per batch)"""
    if case.group == "insert":
        return "add" if route == "add" else "rows"
    return {"stream": "stream", "cache": "stream", "parts": "rows", "many": "rows"}.get(case.group, "add")


def table_batches(case: Case, child: Child, kind: int, how: str):
    """the batches of entries one table of one set receives"""
    if kind == case.kind:
        return [list(b) for b in child.batches]
    if how == "add":
        return []
    if kind == KIND_FIELD:
        return [[b"k"] if b else [] for b in child.batches]
    return [[companion(e, case.kind) for e in b] for b in child.batches]


def table_cap(case: Case, child: Child, kind: int, how: str) -> int:
    if kind == case.kind and child.hint:
        return pow2_at_least(child.hint)
    if kind == KIND_FIELD:
        return DEFAULT_FIELD_SLOTS
    rows = sum(len(b) for b in child.batches) * case.repeat
    return pow2_at_least(max(DEFAULT_TOKEN_SLOTS, 4 * rows)) if how == "rows" else DEFAULT_TOKEN_SLOTS


def batch_growths(batches, cap: int):
    """the growths a table of cap slots is forced to, batch by batch (None: the order decides)"""
    grown, seen = 0, []
    for b in batches:
        seen += b
        g = forced_growths(seen, cap)
        if g is None:
            return None
        cap, grown = cap * GROWTH ** g, grown + g
    return grown


def child_growths(case: Case):
    """per child: the growths its placed table is forced to (None: the order decides)"""
    return [batch_growths(table_batches(case, c, case.kind, "add"), table_cap(case, c, case.kind, "add")) for c in case.children]


def child_tables(case: Case, parent: int):
    return _child_tables(case.name, parent)


@functools.lru_cache(maxsize=None)
def _child_tables(name: str, parent: int):
    """the placed tables of one parent's children as the device holds them at the union: filled in batch order at the capacity the
    forced growths leave"""
    case, out = CASES[name], []
    for c, g in zip(case.children, child_growths(case)):
        if c.parent == parent:
            out.append(tuple(fill([e for b in c.batches for e in b], table_cap(case, c, case.kind, "add") * GROWTH ** g)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _set_growths(name: str, how: str):
    """(exact, lower) over every table of every set of the case"""
    case = CASES[name]
    exact, lower = 0, 0
    for c in case.children:
        for kind in (KIND_FIELD, KIND_TOKEN, KIND_FT):
            g = batch_growths(table_batches(case, c, kind, how), table_cap(case, c, kind, how))
            exact = None if g is None or exact is None else exact + g
            lower += g or 0
    return exact, lower


def predicted_grows(case: Case, route: str):
    """(exact, lower): stats.table_grows of the case under the route — exact where every order gives the same number (then lower is
    the same number), None where it does not; lower is what is certain either way.  Every table counts: the placed one, and on the
    rows routes the field table ("k") and the table of the companions, at their default capacities; then every parent table's union."""
    how = insertion(case, route)
    exact, lower = _set_growths(case.name, how)
    mode, coarsen = ROUTES.get(route, (0, 0))
    # a context of several entries unions every part's sets into the part's own partial parents; the merged tables' growths are not
    # in stats.table_grows (bsg_ingest_stats_read sums the parts'), so the merge adds nothing here
    cuts = parts_cut(case) if case.group == "parts" else [0, len(case.children)]
    retried = False
    for q in range(len(cuts) - 1):
        kids = case.children[cuts[q]: cuts[q + 1]]
        for p in range(case.n_parents):
            for kind in (KIND_FIELD, KIND_TOKEN, KIND_FT):
                mine = [set(e for b in table_batches(case, c, kind, how) for e in b) for c in kids if c.parent == p]
                total = sum(len(s) for s in mine)
                if total == 0:
                    continue
                if mode == 1:                 # union_global_tables: 2 x the children's entries, rounded up
                    g = forced_growths(set().union(*mine), pow2_at_least(max(MIN_CAP, 2 * total)))
                else:
                    g = union_retries(mine, coarsen)
                    # (union_partitioned counts an attempt once however many parent tables it repeats: one table at most may retry here)
                    assert not (g and retried), case.name
                    retried = retried or bool(g)
                exact = None if g is None or exact is None else exact + g
                lower += g or 0
    return exact, lower


def _insert_cases():
    out = []

    def one(name, entries, hint, why, kind=KIND_TOKEN, routes=INSERT_ROUTES, repeat=1, batches=None):
        out.append(Case(name, "insert", kind, (Child(hint, None, batches or (tuple(entries),)),), 0, routes, repeat, why))

    mid, last = 0x5A, 0xFF                                   # a home in the middle of 256 slots, and the last one
    for n in (96, 97, 98):
        one("same-home-%d" % n, cluster("sa", n, 8, mid), 256,
            "n entries of one home: the one that ends at home + j advanced j times, so n <= kMaxProbe + 1 = 97 fits and 98 grows the "
            "table once; at 1 024 slots 2 + 96 lie in two runs")
    one("same-home-98-top-10-bits", cluster("sb", 98, 10, mid << 2 | 1), 256,
        "98 entries sharing 10 key bits are still one home at 1 024 slots: two growths, 256 -> 1 024 -> 4 096")
    for n in (2, 97, 98):
        one("last-home-%d" % n, cluster("sc", n, 8, last), 256,
            "the same at home cap - 1: the cluster continues at slot 0; 98 grow the table once")
    full = place("sd", 65)
    one("full-64-of-64", full[:64], 64, "64 entries into 64 slots: none advances more than 63 times", routes=("add",))
    one("full-64-then-one-more", full, 64,
        "the 65th finds no empty slot and advances 97 times: one growth, whose rehash reads a table without an empty slot; 65 entries "
        "in 256 slots cannot overflow", routes=("add",), batches=(full[:64], full[64:]))
    one("same-home-97-x64", cluster("sa", 97, 8, mid), 256, "every entry 64 times in one call: duplicates do not advance", repeat=64)
    one("same-home-98-x64", cluster("sa", 98, 8, mid), 256, "every entry 64 times in one call: one growth as with one copy each", repeat=64)
    one("full-64-of-64-x64", full[:64], 64, "every entry 64 times in one call: 64 distinct entries fit 64 slots", routes=("add",), repeat=64)
    # the placed cluster is the field::token table's: entry B of set_insert2 has the long chain, A (the token) finishes first
    for n in (97, 98):
        one("ft-same-home-%d" % n, cluster("se", n, 8, mid, KIND_FT), 256,
            "the same-home cluster as k::<word> entries of the field::token table", kind=KIND_FT, routes=INSERT_ROUTES[1:])
    one("ft-last-home-98", cluster("sf", 98, 8, last, KIND_FT), 256,
        "the wrapping cluster as k::<word> entries of the field::token table", kind=KIND_FT, routes=INSERT_ROUTES[1:])
    return out


def _stream_cases():
    c = cluster("sg", 98, 8, 0xFF)
    return [Case("grow-across-appends", "stream", KIND_TOKEN, (Child(256, 0, (c[:97], c[97:])),), 1, ("rows-trusted",), 1,
                 "batch 1 leaves a wrapping cluster of 97 (no growth); batch 2's one entry of the same home makes 98: one growth, "
                 "rehashed from the table")]


def _union_cases():
    out = []

    def one(name, children, n_parents, why, group="union", routes=ALL_ROUTES):
        kids = tuple(Child(h, p, (tuple(es),)) for h, p, es in children)
        out.append(Case(name, group, KIND_TOKEN, kids, n_parents, routes, 1, why))

    any_home = place("ua", 200)
    one("child-full", [(64, 0, any_home[:64]), (64, 0, any_home[32:96])], 1,
        "a child with 64 of 64 slots taken has no gap: the scan makes one lap; its neighbour shares 32 entries")
    wrapped = cluster("ub", 40, 6, 63) + place("uc", 6, top=(6, 0)) + place("ud", 3, top=(6, 1))
    one("child-wraps", [(64, 0, wrapped), (64, 0, wrapped[10:] + any_home[100:110])], 1,
        "40 entries of home 63 continue at slot 0 and push partition 0's and 1's own entries behind them")
    run97 = cluster("ue", 97, 8, 0x21)
    far = tuple(e for e in any_home if 0x90 <= home(hashes(e), 256) < 0xF0)[:20]      # (kept away from the run: its length is then forced)
    assert len(far) == 20
    one("run-97-over-fine-partitions", [(256, 0, run97 + far), (64, 0, run97[:50])], 1,
        "a 97-slot run of one home lies across many partitions' runs: each finds it only through the chain")
    one("capacities-64-256-4096", [(64, 0, any_home[:40]), (256, 0, any_home[20:120]), (4096, 0, any_home[60:200])], 1,
        "one partition's run is a fraction of a slot in one child and several slots in another")
    one("empty-and-single", [(64, 0, ()), (64, 0, any_home[:1]), (256, 0, ()), (64, 0, any_home[1:2])], 1, "an empty child; one entry")
    one("same-in-every-child", [(64, 0, any_home[:50]), (256, 0, any_home[:50]), (64, 0, any_home[:50]), (1024, 0, any_home[:50])], 1,
        "four children with the same 50 entries: the parent holds 50")
    one("disjoint-children", [(64, 0, any_home[:50]), (64, 0, any_home[50:100]), (256, 0, any_home[100:200])], 1, "nothing shared")
    one("parent-without-child", [(64, 0, any_home[:30]), (64, 2, any_home[20:60])], 3, "parent 1 has no child at all")
    # lab key 10 = 4 changes nothing where the default is one partition; here the default is two, the coarse start one partition of
    # more than kPartFill distinct entries, and its retry four
    many = place("uf", 2100)
    one("coarse-start-retries", [(4096, 0, many[:700]), (4096, 0, many[700:1400]), (4096, 0, many[1400:])], 1,
        "2 100 distinct entries: two partitions by default; started 16 x coarser, one partition overflows kPartFill and the retry's "
        "four hold about 525 each", routes=("default", "coarse-then-retry", "global-tables"))
    return out


MANY_WORDS = 150


def _many_children_cases():
    out = []
    for n in (PART_THREADS + 1, 2 * PART_THREADS + 1):
        pool = place("ma", MANY_WORDS)
        kids = tuple(Child(64, 0, ((pool[(7 * i) % MANY_WORDS],),)) for i in range(n))
        out.append(Case("children-%d" % n, "many", KIND_TOKEN, kids, 1, ALL_ROUTES, 1,
                        "%d sets of one row each under one parent: trip %d of the c0 loop; %d distinct words" % (n, (n - 1) // PART_THREADS + 1, MANY_WORDS)))
    return out


def _fill_cases():
    out = []
    pool = place("fa", PART_FILL + 1, top=(1, 0), distinct_lds=True)
    for n in (PART_FILL, PART_FILL + 1):
        es = pool[:n]
        kids = (Child(4096, 0, (es[:512],)), Child(4096, 0, (es[512:1024],)), Child(4096, 0, (es[1024:],)))
        out.append(Case("lds-fill-%d" % n, "fill", KIND_TOKEN, kids, 1, ("default",), 1,
                        "the counts sum to %d: two partitions, and every key's top bit is 0, so partition 0 holds all %d (kPartFill = %d) "
                        "at pairwise different LDS slots: %s" % (n, n, PART_FILL, "no retry" if n == PART_FILL else "one retry, 4 x finer")))
    return out


def _probes_cases():
    out = []
    # 49 of one LDS slot, of which each quarter of the key space holds 12 or 13: 4 x finer no partition has more than 13
    pool = sum((place("pa", 13 if q == 0 else 12, top=(2, q), lds=777) for q in range(4)), ())
    assert len(pool) == PART_PROBES + 1
    for n in (PART_PROBES, PART_PROBES + 1):
        es = pool[:12] + pool[13:] if n == PART_PROBES else pool
        kids = (Child(256, 0, (es[:20],)), Child(256, 0, (es[15:],)))
        out.append(Case("lds-chain-%d" % n, "probes", KIND_TOKEN, kids, 1, ("default",), 1,
                        "%d entries of one partition and one LDS slot: the last advances %d times (kPartProbes = %d): %s"
                        % (n, n - 1, PART_PROBES, "no retry" if n == PART_PROBES else "one retry, after which four partitions hold 13 at most")))
    return out


def collision_pair():
    from tests.test_collisions import pair
    return pair(2)


def _collision_cases():
    a, b = collision_pair()
    kids = (Child(64, 0, ((a,),)), Child(64, 0, ((b,),)))
    return [Case("collision-pair-split", "collision", KIND_TOKEN, kids, 1, ("default", "64-partitions", "global-tables"), 1,
                 "two entries with equal base hashes and different bytes, one per child: each child is clean, their union is flagged")]


def parts_cut(case: Case):
    cost = [sum(len(b) for b in c.batches) * ROW_BYTES + 64 for c in case.children]
    return balanced_cuts(cost, 2)


PART_COUNTS = (1, 63, 64, 65, 257)            # distinct entries of parents 0 .. 4 in the SECOND part
PART_FIRST_OWN = 60                           # entries of every set of the FIRST part that the second part does not hold


def balanced_cuts(cost, parts: int):
    """bsh::balanced_cuts (host/build_plan.hpp), unit 1"""
    cuts, acc, made, total = [0], 0, 1, sum(cost)
    for i, c in enumerate(cost):
        if made >= parts:
            break
        acc += c
        if i + 1 < len(cost) and acc * parts >= total * made:
            cuts.append(i + 1)
            made += 1
    return cuts + [len(cost)]


def _parts_cases():
    """ten sets, parents 0 .. 4 twice: bsg_ingest_rows over a context of two entries cuts them by row bytes + 64 per set — behind set 4
    (parts_cut).  Part 0's partial parents are read in place; part 1's are dense lists of 1, 63, 64, 65 and 257 entries, packed by
    k_table_compact and unioned by k_ingest_union; half of part 1's entries of a parent (rounded down) are in part 0's set of the same
    parent too, beside PART_FIRST_OWN of its own"""
    pool = place("qa", sum(PART_COUNTS) + len(PART_COUNTS) * PART_FIRST_OWN)
    second, at = [], 0
    for n in PART_COUNTS:
        second.append(pool[at: at + n])
        at += n
    first = []
    for es in second:
        first.append(es[: len(es) // 2] + pool[at: at + PART_FIRST_OWN])
        at += PART_FIRST_OWN
    kids = [Child(0, p, (tuple(es),)) for p, es in enumerate(first)] + [Child(0, p, (tuple(es),)) for p, es in enumerate(second)]
    return [Case("two-parts", "parts", KIND_TOKEN, tuple(kids), len(PART_COUNTS), ("rows-trusted",), 1,
                 "per-part partial parents of 1, 63, 64, 65 and 257 entries with duplicates across the parts")]


def _cache_cases():
    """rows of two sets alternating row by row in one append: row r belongs to set r % 2 and holds word (r // 2) % n of its set's list.
    Every word shares ONE set of the 2-way dedup cache, so the ways are evicted all the time, and the sets share words: only the
    tag tells the tables apart"""
    out = []
    w = place("ca", 4, cache=123)
    for name, lists in (("cache-3-shared", (w[:3], w[:3])), ("cache-4-shared", (w, w)), ("cache-4-overlap", (w[:3], w[1:]))):
        kids = tuple(Child(0, 0, (tuple(ws),)) for ws in lists)
        out.append(Case(name, "cache", KIND_TOKEN, kids, 1, ("rows-trusted",), 40,
                        "%d and %d words of one cache set, 40 rows each, the two sets' rows alternating inside one workgroup"
                        % (len(lists[0]), len(lists[1]))))
    return out


def _table():
    cases = (_insert_cases() + _stream_cases() + _union_cases() + _many_children_cases() + _fill_cases() + _probes_cases()
             + _collision_cases() + _parts_cases() + _cache_cases())
    table = {c.name: c for c in cases}
    assert len(table) == len(cases)
    return table


CASES = _table()
SCAN_GROUPS = ("union", "many", "fill", "probes")          # the groups whose children the scan model is run over


def scan_log2ps(case: Case):
    return _scan_log2ps(case.name)


@functools.lru_cache(maxsize=None)
def _scan_log2ps(name: str):
    """the partition counts (as log2) the case's routes give the placed table's parent 0"""
    case = CASES[name]
    mine = [s for s, c in zip(child_sets(case), case.children) if c.parent == 0]
    total, out = sum(len(s) for s in mine), set()
    for r in case.routes:
        if ROUTES[r][0] == 0:
            lg = route_log2p(total, ROUTES[r][1])
            out |= {lg, lg + 2 * (union_retries(mine, ROUTES[r][1]) or 0)}      # the attempt that overflows, and the one that does not
    return sorted(out)


def cache_rows(case: Case):
    """(rows, set_of_row) of a cache case's one append"""
    rows, sor = [], []
    lists = [c.batches[0] for c in case.children]
    for r in range(2 * case.repeat * max(len(ws) for ws in lists)):
        ws = lists[r % 2]
        if r // 2 < case.repeat * len(ws):
            rows.append(row_of(ws[(r // 2) % len(ws)], case.kind))
            sor.append(r % 2)
    return rows, sor
