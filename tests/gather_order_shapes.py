"""The gather kernels' order of a lane's k locations and their phase walk, restated in plain Python from the oracle's hashes and
location arithmetic (no numpy tricks, nothing shared with tools/probe_gather_lab.py, which the CPU test compares it with).

A lane owns one term of a block's filter (m bits, k locations).  ORDER:
  "index"  the locations in hash-index order
  "line"   by (loc >> 10, hash index): ascending 128-byte span of the filter, ties by hash index — the shipped order for filters of
           m < 2^31 bits (the 32-bit modulo), m <= ORDER_MAX_M and k <= ORDER_MAX_K; every other filter keeps the index order
PHASES: the lane takes its ordered locations in phases of SCHEDULE's lengths (the last length repeats, every phase is clipped at k); it
runs a phase iff every bit of its earlier phases was set, and it executes every test of a phase it runs.  The verdict is the AND of
all k bits whatever the order.  A nil filter (m = 0) executes nothing and passes."""
from oracle import oracle as O

SCHEDULE = (1, 3, 6)
ORDER_MAX_K = 16
ORDER_MAX_M = 1 << 27
SHIPPED = "line"


def locations(h, m, k):
    return [O.location(h, i) % m for i in range(k)]


def ordered(locs, m, order):
    """-> the hash indices in the order the lane tests them"""
    k = len(locs)
    if order == "line" and m < (1 << 31) and m <= ORDER_MAX_M and k <= ORDER_MAX_K:
        return sorted(range(k), key=lambda i: (locs[i] >> 10, i))
    assert order in ("line", "index"), order
    return list(range(k))


def phases(k, schedule=SCHEDULE):
    """-> [(first position, length)] of the phases up to k"""
    out, at, p = [], 0, 0
    while at < k:
        n = min(schedule[min(p, len(schedule) - 1)], k - at)
        out.append((at, n))
        at += n
        p += 1
    return out


def bit_set(words, d, loc):
    return (int(words[int(d["word_off"]) + (loc >> 6)]) >> (loc & 63)) & 1


def walk_lane(words, d, h, order=SHIPPED, schedule=SCHEDULE):
    """one term against one filter descriptor -> (tests executed, passed, [(phase, arena line)] of the executed tests)"""
    m, k = int(d["m"]), int(d["k"])
    if m == 0:
        return 0, True, []
    locs = locations(h, m, k)
    seq = ordered(locs, m, order)
    tests, alive, touched = 0, True, []
    for p, (at, n) in enumerate(phases(k, schedule)):
        if not alive:
            break
        for i in seq[at: at + n]:
            tests += 1
            touched.append((p, (int(d["word_off"]) * 8 + (locs[i] >> 3)) >> 7))
            alive = alive and bool(bit_set(words, d, locs[i]))
    return tests, alive, touched


def walk_arena(words, desc, term_strings, kinds, order=SHIPPED, schedule=SCHEDULE):
    """-> per block: tests executed, distinct lines touched, sum over the phases of the phase's distinct lines, [verdict per term]"""
    hs = [O.base_hashes(s if isinstance(s, bytes) else s.encode()) for s in term_strings]
    out = []
    for b in range(len(desc) // 3):
        tests, touched, verdicts = 0, [], []
        for h, kind in zip(hs, kinds):
            t, ok, tl = walk_lane(words, desc[b * 3 + int(kind)], h, order, schedule)
            tests += t
            touched += tl
            verdicts.append(ok)
        out.append((tests, len({ln for _, ln in touched}), len(set(touched)), verdicts))
    return out


def a_word_with_two_equal_locations(m, k, prefix="w", limit=200000):
    """-> a lower-case string two of whose k locations in a filter of m bits coincide (and the two hash indices)"""
    for n in range(limit):
        s = prefix + "".join(chr(97 + (n // 26 ** j) % 26) for j in range(4))
        locs = locations(O.base_hashes(s.encode()), m, k)
        seen = {}
        for i, loc in enumerate(locs):
            if loc in seen:
                return s, seen[loc], i
            seen[loc] = i
    raise AssertionError("no such word among %d" % limit)
