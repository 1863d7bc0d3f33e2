"""The arithmetic of the row-matcher calls on the host (no GPU): tests/wide_plan_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/wide_plan.hpp, compared with restatements written here from the call's contract (include/bloomgpu.h):
where a pair's words lie, which conditions a set's queries reference, where a call is cut between devices, a part's sets and the
evaluation kernel's work items; and, for the single and batched calls that share the cuts and the set range, against restatements of
the loops those calls had of their own.  What the callers rely on is asserted by itself too: every (pair, tile) word of a part is written
by exactly one item, cuts lie at set-relative multiples of 64 rows, and the parts' words scatter to the call's layout without
overlap."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, SET_SPAN, SET_ORDER, PAIR_ORDER = range(5)
ITEM_PAIRS = 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wide_plan") / "wide_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "wide_plan_check.cpp")],
                   check=True, timeout=300)
    return exe


class Answers:
    def __init__(self, words):
        self.w, self.at = words, 0

    def take(self, n=None):
        if n is None:
            self.at += 1
            return int(self.w[self.at - 1])
        self.at += n
        return [int(x) for x in self.w[self.at - n: self.at]]

    def done(self):
        return self.at == len(self.w)


def run_driver(exe, tmp_path, cases):
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8")] + [np.asarray(c, dtype="<u8") for c in cases])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return Answers(np.fromfile(tmp_path / "answers.bin", dtype="<u8"))


def tiles(n):
    return -(-n // 64)


def test_the_header_states_the_calls_limits(driver, tmp_path):
    ans = run_driver(driver, tmp_path, [[0]])
    max_q, max_ops, max_pairs, max_items, item_pairs, lds_cap, item_bytes = ans.take(7)
    assert ans.done()
    assert max_q >= 65536 and max_ops >= 1 << 20 and max_pairs >= 1 << 24             # what the call must at least hold
    from bloomsearch_amd import query as Q
    assert (max_q, max_ops, max_pairs) == (Q.MATCH_WIDE_MAX_QUERIES, Q.MATCH_WIDE_MAX_OPS, Q.MATCH_WIDE_MAX_PAIRS)
    assert item_pairs == ITEM_PAIRS and item_bytes == 32 and max_items == 1 << 30
    # the table cap follows from the storing walker's LDS: 80 KiB (two workgroups per CU) minus conditions 64 * 11 * 8 and 256 lanes * 116
    hdr = open(os.path.join(ROOT, "include", "bloomgpu.h")).read()
    assert lds_cap == 80 * 1024 - (64 * 11 * 8 + 256 * 116) == 46592 and "46 592" in hdr


def want_pair_words(first, off):
    pwo, at = [], 0
    for s in range(len(first) - 1):
        for _ in range(off[s], off[s + 1]):
            pwo.append(at)
            at += tiles(first[s + 1] - first[s])
    return pwo + [at], at


def test_pair_words(driver, tmp_path):
    sizes = [0, 1, 63, 64, 65, 0, 130, 64, 1]
    first = [0] + list(np.cumsum(sizes))
    off = [0, 2, 2, 5, 6, 6, 9, 79, 79, 80]                                            # sets with no pair: 1 (1 row), 4 (65 rows), 7 (64 rows)
    n_rows, n_sets = first[-1], len(sizes)
    good = [1, n_sets, n_rows, 100, 1, 1, 1] + first + off
    cases = [good, [1, n_sets, n_rows, 100, 1, 1, 0] + first + off]
    for n, q in ((0, 0), (1, 1), (63, 3), (64, 2), (65, 70), (257, 0)):                # the implicit set
        cases.append([1, 0, n, q, 0, 0, 1])
    bad_first = list(first)
    bad_first[3], bad_first[4] = first[4], first[3]
    bad_off = list(off)
    bad_off[5] = 10
    malformed = [([1, n_sets, n_rows, 100, 0, 1, 1] + off, NULL), ([1, n_sets, n_rows, 100, 1, 0, 1] + first, NULL),
                 ([1, 0, n_rows, 100, 1, 0, 1, 0], NULL),                                  # a table without its number of sets
                 ([1, n_sets, n_rows + 1, 100, 1, 1, 1] + first + off, SET_SPAN), ([1, n_sets, n_rows, 100, 1, 1, 1] + [1] + first[1:] + off, SET_SPAN),
                 ([1, n_sets, n_rows, 100, 1, 1, 1] + bad_first + off, SET_ORDER), ([1, n_sets, n_rows, 100, 1, 1, 1] + first + bad_off, PAIR_ORDER),
                 ([1, n_sets, n_rows, 100, 1, 1, 1] + first + [1] + off[1:], PAIR_ORDER)]
    ans = run_driver(driver, tmp_path, cases + [c for c, _ in malformed])
    pwo, total = want_pair_words(first, off)
    assert ans.take() == OK and ans.take() == total and ans.take() == len(pwo) and ans.take(len(pwo)) == pwo
    assert ans.take() == OK and ans.take() == total and ans.take() == 0
    assert total == 2 * 0 + 3 * 1 + 1 * 1 + 3 * 0 + 70 * 3 + 1 * 1
    for n, q in ((0, 0), (1, 1), (63, 3), (64, 2), (65, 70), (257, 0)):
        assert ans.take() == OK and ans.take() == q * tiles(n) and ans.take() == q + 1
        assert ans.take(q + 1) == [i * tiles(n) for i in range(q + 1)]                 # the planes of bsg_match_rows_many
    for _, status in malformed:
        assert ans.take() == status
    assert ans.done()


def random_programs(rng, n_queries, n_conds):
    ops, poff, masks = [], [0], []
    for _ in range(n_queries):
        m = 0
        for _ in range(int(rng.integers(0, 6))):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                c = int(rng.integers(0, n_conds))
                ops.append(c)                                                          # TERM c: opcode 0
                m |= 1 << c
            else:
                ops.append((int(rng.integers(1, 5)) << 28) | int(rng.integers(0, 64)))    # AND / OR / TRUE / FALSE: their argument is no condition
        masks.append(m)
        poff.append(len(ops))
    return ops, poff, masks


def test_condition_masks(driver, tmp_path):
    rng = np.random.default_rng(4)
    cases, wants = [], []
    for n_conds, n_queries, n_sets in ((1, 1, 1), (64, 300, 7), (29, 4096, 40), (5, 0, 2)):
        ops, poff, qm = random_programs(rng, n_queries, n_conds)
        sqo, sq, sm = [0], [], []
        for s in range(n_sets):
            listed = sorted(int(q) for q in rng.choice(n_queries, size=int(rng.integers(0, min(n_queries, 90) + 1)), replace=False)) if n_queries and s != 1 else []
            sq += listed
            sqo.append(len(sq))
            m = 0
            for q in listed:
                m |= qm[q]
            sm.append(m)
        cases.append([2, n_conds, n_queries] + poff + ops + [n_sets] + sqo + sq)
        wants.append(qm + sm)
    ans = run_driver(driver, tmp_path, cases)
    for w in wants:
        assert ans.take(len(w)) == w
    assert ans.done()
    assert any(m >> 63 for m in wants[1])                                              # condition 63 is a mask bit like any other


def want_parts(row_off, first, sqo, want):
    """the cuts by the contract: near the byte targets, moved down to a set-relative multiple of 64 rows"""
    n_rows = len(row_off) - 1
    cuts = [0]
    total = row_off[-1] - row_off[0]
    for i in range(1, want):
        target = row_off[0] + total * i // want
        r = int(np.searchsorted(np.asarray(row_off[:n_rows], dtype=np.uint64), target, side="left"))
        s = max(k for k in range(len(first) - 1) if first[k] <= r)                     # a target inside the last row: the last set's last tile boundary
        r = first[s] + (r - first[s]) // 64 * 64
        if cuts[-1] < r < n_rows:
            cuts.append(r)
    return cuts + [n_rows]


def test_parts_and_items(driver, tmp_path):
    rng = np.random.default_rng(9)
    shapes = []
    for sizes, want in (([1], 3), ([63, 64, 65, 1, 0, 130], 1), ([63, 64, 65, 1, 0, 130], 2), ([300, 0, 7, 1000, 129], 3), ([5000], 8),
                        ([int(x) for x in rng.integers(0, 400, size=30)], 4)):
        first = [0] + [int(x) for x in np.cumsum(sizes)]
        n_rows = first[-1]
        row_off = [7] + [int(x) for x in 7 + np.cumsum(rng.integers(1, 300, size=n_rows))]
        sqo = [0]
        for s in range(len(sizes)):
            sqo.append(sqo[-1] + (0 if s % 4 == 1 else int(rng.integers(1, 150))))
        shapes.append((row_off, first, sqo, want))
    ans = run_driver(driver, tmp_path, [[3, len(ro) - 1] + ro + [len(f) - 1] + f + o + [w] for ro, f, o, w in shapes])
    cut_inside_a_set = 0
    for row_off, first, sqo, want in shapes:
        n_sets = len(first) - 1
        cuts = ans.take(ans.take())
        assert cuts == want_parts(row_off, first, sqo, want)
        pwo, total = want_pair_words(first, sqo)
        written = np.zeros(total, dtype=np.int64)
        for r0, r1 in zip(cuts, cuts[1:]):
            s0, n = ans.take(), ans.take()
            first_row, pair_off, tile0 = ans.take(n + 1), ans.take(n + 1), ans.take(n)
            ok, words, n_items = ans.take(), ans.take(), ans.take()
            items = [ans.take(6) for _ in range(n_items)]
            # the part's sets: from the first to the last set with a row in [r0, r1), clamped; r0 a whole number of its set's tiles
            with_rows = [s for s in range(n_sets) if max(first[s], r0) < min(first[s + 1], r1)]
            sets = list(range(with_rows[0], with_rows[-1] + 1))                          # an empty set between them comes along (no rows, no items)
            assert ok == 1 and (s0, n) == (sets[0], len(sets)) and sets == list(range(s0, s0 + n))
            assert first_row == [max(first[s], r0) - r0 for s in sets] + [r1 - r0]
            assert pair_off == [sqo[s] for s in sets] + [sqo[sets[-1] + 1]]
            assert tile0 == [(max(first[s], r0) - first[s]) // 64 for s in sets]
            assert all((max(first[s], r0) - first[s]) % 64 == 0 for s in sets)
            cut_inside_a_set += first[s0] < r0
            # the items: each (local pair, local tile) exactly once, rows of one set, at most 64 pairs
            local = np.zeros(words, dtype=np.int64)
            at = 0
            base = {}
            for ls, s in enumerate(sets):
                base[ls] = at
                at += tiles(first_row[ls + 1] - first_row[ls]) * (sqo[s + 1] - sqo[s])
            assert at == words
            for out0, row0, n_item_rows, p0, p1, stride in items:
                ls = max(k for k in range(n) if first_row[k] <= row0 and first_row[k] < first_row[k + 1])
                s = sets[ls]
                t, rem = divmod(row0 - first_row[ls], 64)
                assert rem == 0 and 1 <= n_item_rows <= 64 and n_item_rows == min(64, first_row[ls + 1] - row0)
                assert stride == tiles(first_row[ls + 1] - first_row[ls]) and 0 < p1 - p0 <= ITEM_PAIRS
                assert sqo[s] - pair_off[0] <= p0 and p1 <= sqo[s + 1] - pair_off[0]
                for p in range(p0, p1):
                    w = out0 + (p - p0) * stride
                    assert w == base[ls] + (p - (sqo[s] - pair_off[0])) * stride + t
                    local[w] += 1
                    written[pwo[p + pair_off[0]] + tile0[ls] + t] += 1                  # where the host scatters it to
            assert (local == 1).all()
        assert (written == 1).all()                                                    # no two parts write one word of the call
    assert ans.done() and cut_inside_a_set >= 3


def old_plane_cuts(row_off, want):
    """the cut loop match_rows_run had for the single and batched calls: byte targets, moved down to a multiple of 64 rows"""
    n_rows = len(row_off) - 1
    n_bytes = row_off[-1] - row_off[0]
    cuts = [0]
    for i in range(1, want):
        target = row_off[0] + n_bytes * i // want
        r = 0                                                                          # std::lower_bound(row_off, row_off + n_rows, target)
        while r < n_rows and row_off[r] < target:
            r += 1
        r = r // 64 * 64
        if cuts[-1] < r < n_rows:
            cuts.append(r)
    return cuts + [n_rows]


def plane_cut_shapes():
    rng = np.random.default_rng(21)
    shapes = []
    for n_rows in (1, 63, 64, 65, 129, 4097):
        uniform = [3] + [3 + 100 * (r + 1) for r in range(n_rows)]
        lens = rng.integers(1, 40, size=n_rows)
        lens[rng.integers(0, n_rows, size=max(1, n_rows // 50))] = 50000                # a few rows hold most of the bytes
        skewed = [0] + [int(x) for x in np.cumsum(lens)]
        last = [0] + [int(x) for x in np.cumsum([10] * (n_rows - 1) + [10 ** 6])]      # every target falls into the last row
        head = [0] + [int(x) for x in np.cumsum([10 ** 6] + [10] * (n_rows - 1))]      # ... into the first
        for row_off in (uniform, skewed, last, head):
            for want in (1, 2, 3, 8):
                shapes.append((row_off, want))
    # two targets in one 64-row block: rows 70 and 100 hold the thirds of the bytes, both move down to row 64
    lens = [1] * 129
    lens[70] = lens[100] = 10 ** 5
    shapes.append(([0] + [int(x) for x in np.cumsum(lens)], 3))
    return shapes


def test_the_plane_calls_cuts_are_the_cuts_of_one_implicit_set(driver, tmp_path):
    shapes = plane_cut_shapes()
    ans = run_driver(driver, tmp_path, [[4, len(ro) - 1] + ro + [w] for ro, w in shapes])
    seen = set()
    for row_off, want in shapes:
        cuts = ans.take(ans.take())
        assert cuts == old_plane_cuts(row_off, want), (len(row_off) - 1, want)
        assert all(c % 64 == 0 for c in cuts[:-1]) and cuts == sorted(set(cuts))
        seen.add(len(cuts) - 1)
    assert ans.done() and {1, 2, 3, 8} <= seen
    assert old_plane_cuts(shapes[-1][0], 3) == [0, 64, 129]                            # the second target's cut is dropped, not repeated
    last_129 = [0] + [int(x) for x in np.cumsum([10] * 128 + [10 ** 6])]
    assert old_plane_cuts(last_129, 2) == [0, 128, 129]                                # a target inside the last row still cuts


def old_set_clamp(first, r0, r1):
    """the clamp loop match_rows_on had: the sets rows [r0, r1) lie in, their first rows clamped to the run and counted from r0"""
    n_sets = len(first) - 1
    s0 = 0                                                                             # std::upper_bound(sf + 1, sf + n_sets + 1, r0) - (sf + 1)
    while s0 < n_sets and first[s0 + 1] <= r0:
        s0 += 1
    s1 = 0                                                                             # std::lower_bound(sf, sf + n_sets, r1) - sf
    while s1 < n_sets and first[s1] < r1:
        s1 += 1
    return s0, [min(max(first[s0 + i], r0), r1) - r0 for i in range(s1 - s0 + 1)]


def test_a_parts_set_range_is_the_batched_calls_clamp(driver, tmp_path):
    sizes = [0, 0, 64, 1, 0, 0, 130, 63, 0, 65, 0]                                     # empty sets at both ends and in the middle
    first = [0] + [int(x) for x in np.cumsum(sizes)]
    n_rows = first[-1]
    ranges = [(0, n_rows), (0, 64), (64, 65), (64, 128), (65, 195), (128, 192), (100, 101), (0, 1), (n_rows - 1, n_rows), (195, 258), (258, n_rows),
              (192, n_rows), (63, 66), (1, 64)]                                         # inside a set, on set boundaries, across empty sets
    ranges += [(r0, r1) for r0 in range(0, n_rows, 37) for r1 in range(r0 + 1, n_rows + 1, 41)]
    shapes = [(first, r0, r1) for r0, r1 in ranges] + [([0, 5], 0, 5), ([0, 5], 2, 3), ([0, 0, 5, 5], 0, 5)]
    ans = run_driver(driver, tmp_path, [[5, len(f) - 1] + f + [r0, r1] for f, r0, r1 in shapes])
    for f, r0, r1 in shapes:
        s0, n = ans.take(), ans.take()
        first_row = ans.take(n + 1)
        assert (s0, first_row) == old_set_clamp(f, r0, r1), (r0, r1)
        assert first_row[0] == 0 and first_row[-1] == r1 - r0 and first_row == sorted(first_row)
    assert ans.done()


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    """the same driver as a stand-alone program under AddressSanitizer and UBSan, over every kind of case"""
    exe = tmp_path / "wide_plan_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "wide_plan_check.cpp")],
                   check=True, timeout=300)
    first, off = [0, 0, 1, 64, 128, 193, 323], [0, 3, 3, 4, 74, 75, 145]
    row_off = list(range(0, 324 * 50, 50))
    cases = [[0], [1, 6, 323, 80, 1, 1, 1] + first + off, [1, 0, 65, 3, 0, 0, 1], [1, 6, 322, 80, 1, 1, 1] + first + off,
             [2, 3, 2, 0, 2, 3, 0, 2, 1, 2, 0, 1, 2, 0, 1], [3, 323] + row_off + [6] + first + off + [3],
             [4, 323] + row_off + [3], [5, 6] + first + [64, 200]]
    ans = run_driver(exe, tmp_path, cases)
    assert ans.take(7)[5] == 46592
