"""The arithmetic of the write side on the host (no GPU): tests/build_plan_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/build_plan.hpp — the code bsg_arena_load, plan_arena and stream_finish lay a shard out and fold its
stats by, build_common and ingest_build_common cut a build call into parts by, and both build routes choose a filter's route by.
Reference for every comparison: the loops that header replaced, restated below from bloomsearch_amd/csrc/bloomgpu.hip,
ingest_api.inc, stream_api.inc and encode_api.inc as they stood at commit dc10345 (the line numbers are those files'), when each
route and each of the three shard sites carried a copy of its own.  Every restatement records which of its branches ran, and the
tests assert that all of them did.  On top of the comparison, what the callers rely on is asserted by itself: a shard's filters
are 128-byte aligned and do not overlap; the parts' word ranges are pairwise disjoint whenever the layout ascends; the region
offsets tile [0, total)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LDS_BUDGET = 144 * 1024                     # bloomgpu.hip:88
K_LDS_CAP_WORDS = K_LDS_BUDGET // 8           # bloomgpu.hip:89
K_ALIGN_WORDS = 16                            # bloomgpu.hip:90
K_BIN_SCRATCH_BYTES = 16 << 30                # bloomgpu.hip:92


def _ingest_constant(name, known):
    """a `constexpr uint32_t NAME = <expression>;` of ingest.hip.h, evaluated over the constants read before it"""
    import re
    src = open(os.path.join(ROOT, "bloomsearch_amd", "csrc", "ingest.hip.h")).read()
    expr = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([^;]+);" % name, src).group(1)
    assert re.fullmatch(r"[\w\s*+()-]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}, known))


# ingest.hip.h:1363, 1369, 1370, read from the source: kBuildSetsThreads = 1024, kSetTile = 4 * kBuildSetsThreads, kSetListBytes = kSetTile * 4 + 16
_K = {}
for _name in ("kBuildSetsThreads", "kSetTile", "kSetListBytes"):
    _K[_name] = _ingest_constant(_name, _K)
K_SET_LIST_BYTES = _K["kSetListBytes"]
BIN_MIN_LOCS = 4 << 20                        # bloomgpu.hip:450
POISON = 0xA5A5A5A5A5A5A5A5
STAGED, BINNED, SLICED = 0, 1, 2


# ---- the parent's loops, restated ----

def shard_blocks_before(n_blocks, di, nd):
    """bloomgpu.hip:1301, ingest_api.inc:882, stream_api.inc:219"""
    return (n_blocks - di + nd - 1) // nd if n_blocks > di else 0


def new_stats():
    return {"sum_words": [0] * 3, "max_staged_words": [0] * 3, "fixed_m": [0] * 3, "fixed_k": [0] * 3, "geometry_uniform": [1] * 3}


def fold_before(s, c, m, k, took):
    """the four lines at bloomgpu.hip:1316-1319, ingest_api.inc:898-901 and stream_api.inc:315-318 (each behind `if (f.m == 0) continue`)"""
    if m == 0:
        took.add("nil")
        return
    nw = (m + 63) // 64
    s["sum_words"][c] += nw
    if nw <= K_LDS_CAP_WORDS:
        took.add("stageable")
        s["max_staged_words"][c] = max(s["max_staged_words"][c], nw)
    else:
        took.add("beyond-lds")
    if s["fixed_m"][c] == 0 and s["geometry_uniform"][c]:
        took.add("adopt")
        s["fixed_m"][c], s["fixed_k"][c] = m, k
    elif s["fixed_m"][c] != m or s["fixed_k"][c] != k:
        took.add("mismatch-m" if s["fixed_m"][c] != m else "mismatch-k")
        s["geometry_uniform"][c] = 0
    else:
        took.add("match")


def arena_load_shard_before(desc, n_blocks, di, nd, took):
    """bloomgpu.hip:1298-1322 (bsg_arena_load): local filters (word_off, m, k), n_words, stats"""
    n_local = shard_blocks_before(n_blocks, di, nd)
    dd, s, cursor = [], new_stats(), 0
    for lb in range(n_local):
        b = lb * nd + di
        for c in range(3):
            _, m, k = desc[b * 3 + c]
            o = [0, m, k]
            dd.append(o)
            fold_before(s, c, m, k, took)
            if m == 0:
                continue
            nw = (m + 63) // 64
            o[0] = cursor
            cursor += (nw + K_ALIGN_WORDS - 1) // K_ALIGN_WORDS * K_ALIGN_WORDS
    return n_local, cursor + K_ALIGN_WORDS, dd, s


def plan_arena_shard_before(desc, n_blocks, di, nd):
    """ingest_api.inc:880-905 (plan_arena): the same, and dst_off per local block"""
    n_local = shard_blocks_before(n_blocks, di, nd)
    dd, dst_off, s, cursor = [], [], new_stats(), 0
    for lb in range(n_local):
        b = lb * nd + di
        dst_off.append(cursor)
        at = cursor
        for c in range(3):
            _, m, k = desc[b * 3 + c]
            o = [0, m, k]
            dd.append(o)
            fold_before(s, c, m, k, set())
            if m == 0:
                continue
            o[0] = at
            at += ((m + 63) // 64 + K_ALIGN_WORDS - 1) // K_ALIGN_WORDS * K_ALIGN_WORDS
        cursor = at
    return n_local, cursor + K_ALIGN_WORDS, dd, dst_off, s


def block_span_words_before(d3):
    """ingest_api.inc:865-870"""
    return sum(((m + 63) // 64 + K_ALIGN_WORDS - 1) // K_ALIGN_WORDS * K_ALIGN_WORDS for _, m, _ in d3 if m)


def section_len_before(d3):
    """encode_api.inc:6-12"""
    return 1 + 4 + sum(4 + 24 + 8 * ((m + 63) // 64) for _, m, _ in d3 if m)


def ascending_before(desc):
    """bloomgpu.hip:1208-1215 and ingest_api.inc:1103-1110"""
    prev_end = 0
    for off, m, _ in desc:
        if m == 0:
            continue
        if off < prev_end:
            return False
        prev_end = off + (m + 63) // 64
    return True


def entries_parts_before(desc, ranges, n_words, sections, took):
    """bloomgpu.hip:1224-1242 (build_common): per part (w_lo, w_hi, region_off, region_len); the region total"""
    out, region_cursor = [], 0
    for i0, i1 in ranges:
        lo, hi = None, 0
        for off, m, _ in desc[i0:i1]:
            if m == 0:
                continue
            lo = off if lo is None else min(lo, off)
            hi = max(hi, off + (m + 63) // 64)
        if lo is None:
            took.add("part-of-nil-filters")
            lo = hi = 0
        if len(ranges) == 1:
            took.add("single-part")
            lo, hi = 0, n_words
        region_off = region_len = 0
        if sections:
            region_off = region_cursor
            region_len = sum(section_len_before(desc[b * 3: b * 3 + 3]) for b in range(i0 // 3, i1 // 3))
            region_cursor += region_len
        out.append((lo, hi, region_off, region_len))
    return out, region_cursor


def tables_parts_before(desc, ranges, n_words, sections):
    """ingest_api.inc:1114-1133 (ingest_build_common): regions with sections, word ranges without"""
    out, region_cursor = [], 0
    for i0, i1 in ranges:
        lo = hi = region_off = region_len = 0
        if sections:
            region_off = region_cursor
            region_len = sum(section_len_before(desc[b * 3: b * 3 + 3]) for b in range(i0 // 3, i1 // 3))
            region_cursor += region_len
        elif len(ranges) == 1:
            lo, hi = 0, n_words
        else:
            present = [(off, m) for off, m, _ in desc[i0:i1] if m]
            if present:
                lo, hi = min(off for off, _ in present), max(off + (m + 63) // 64 for off, m in present)
        out.append((lo, hi, region_off, region_len))
    return out, region_cursor


def zero_fill_before(words, n_words, parts, took):
    """bloomgpu.hip:1245-1249 and ingest_api.inc:1136-1140"""
    at = 0
    for n, (lo, hi, _, _) in enumerate(parts):
        if lo > at:
            took.add("gap-before" if n == 0 else "gap-between")
            words[at:lo] = 0
        at = max(at, hi)
    if n_words > at:
        took.add("gap-behind")
        words[at:n_words] = 0


def scatter_before(sec_off, ranges, parts, local):
    """bloomgpu.hip:1256-1259 and ingest_api.inc:1160-1163"""
    for (i0, i1), (_, _, region_off, _), loc in zip(ranges, parts, local):
        for b in range((i1 - i0) // 3 + 1):
            sec_off[i0 // 3 + b] = region_off + loc[b]


def binned_build_fits_before(m, n_entries, k, bin_min_locs, bin_scratch_bytes, took):
    """bloomgpu.hip:1054-1059"""
    n_locs = n_entries * k
    for name, ok in (("m-below-2^31", m < (1 << 31)), ("enough-locs", n_locs >= max(bin_min_locs, 1)),
                     ("locs-below-2^32-4096", n_locs < (1 << 32) - 4096), ("locs-fit-scratch", n_locs * 4 <= bin_scratch_bytes)):
        if not ok:
            took.add("not:" + name)
            return False
    return True


def entries_route_before(m, n_entries, k, bin_min_locs, bin_scratch_bytes, took):
    """bloomgpu.hip:1089-1098 (build_on_device)"""
    nw = (m + 63) // 64
    if nw <= K_LDS_CAP_WORDS:
        return STAGED
    return BINNED if binned_build_fits_before(m, n_entries, k, bin_min_locs, bin_scratch_bytes, took) else SLICED


def tables_route_before(m, n_entries, k, bin_min_locs, bin_scratch_bytes, took):
    """ingest_api.inc:987-996 (build_part)"""
    nw = (m + 63) // 64
    if nw * 8 + K_SET_LIST_BYTES <= K_LDS_BUDGET:
        return STAGED
    return BINNED if binned_build_fits_before(m, n_entries, k, bin_min_locs, bin_scratch_bytes, took) else SLICED


def balanced_cuts_before(cost, parts, unit):
    """bloomgpu.hip:570-584"""
    n, cuts, total, acc, made = len(cost), [0], sum(cost), 0, 1
    for i in range(n):
        if made >= parts:
            break
        acc += cost[i]
        if (i + 1) % unit == 0 and i + 1 < n and acc * parts >= total * made:
            cuts.append(i + 1)
            made += 1
    cuts.append(n)
    return cuts


# ---- the driver ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("build_plan") / "build_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "build_plan_check.cpp")],
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
    """cases: lists of u64 words, each starting with its kind"""
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8")] + [np.asarray(c, dtype="<u8") for c in cases])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return Answers(np.fromfile(tmp_path / "answers.bin", dtype="<u8"))


def desc_words(desc):
    return [len(desc)] + [x for f in desc for x in f]


def test_the_header_states_the_librarys_constants(driver, tmp_path):
    ans = run_driver(driver, tmp_path, [[4]])
    assert ans.take(4) == [K_LDS_BUDGET, K_LDS_CAP_WORDS, K_ALIGN_WORDS, K_SET_LIST_BYTES] and ans.done()
    # the head of the tables route is what ingest.hip.h says (bloomgpu.hip static_asserts the header's copy against it as well)
    assert _K == {"kBuildSetsThreads": 1024, "kSetTile": 4096, "kSetListBytes": 16400}
    assert 0 < K_SET_LIST_BYTES < K_LDS_BUDGET and K_SET_LIST_BYTES % 8 == 0
    assert K_LDS_BUDGET % 8 == 0              # so that a head of 0 bytes reproduces `nw <= kLdsCapWords` exactly


# ---- shard layout and stats ----

CAP_BITS = K_LDS_CAP_WORDS * 64
EDGE_M = [1, 63, 64, 65, 1023, 1024, 1025, 5 * 1024 - 1, 5 * 1024, 5 * 1024 + 1, CAP_BITS - 1, CAP_BITS, CAP_BITS + 1, CAP_BITS + 64, 3 * CAP_BITS]


def shard_scenarios(n_blocks):
    """name -> [(word_off, m, k)] x 3 n_blocks (word_off: the caller's packed layout, not read by the shard layout)"""
    rng = np.random.default_rng(20261017 + n_blocks)
    out = {}
    out["uniform"] = [(0, (9000, 70000, 400000)[c], (7, 10, 10)[c]) for _ in range(n_blocks) for c in range(3)]
    out["mix-m"] = [(0, (9000, 70000 + 64 * (b % 3 == 2), 400000)[c], 7) for b in range(n_blocks) for c in range(3)]
    out["mix-k"] = [(0, (9000, 70000, 400000)[c], 7 + (c == 2 and b % 4 == 3)) for b in range(n_blocks) for c in range(3)]
    # the first blocks' filters of kinds 0 and 2 are nil (on every device of up to 8), one later block is nil altogether
    out["first-nil"] = [(0, 0 if (c != 1 and b < 8) or b == 11 else (9000, 70000, 400000)[c], 10) for b in range(n_blocks) for c in range(3)]
    out["edges"] = [(0, EDGE_M[(b * 3 + c) % len(EDGE_M)], 1 + (b + c) % 3) for b in range(n_blocks) for c in range(3)]
    out["random"] = [(0, int(rng.choice([0, 0, 1000, 1024, 65536, CAP_BITS, CAP_BITS + 1, int(rng.integers(1, 1 << 22))])), int(rng.integers(1, 4)))
                     for _ in range(n_blocks * 3)]
    return out


def shard_cases():
    cases = []
    for nd in (1, 2, 3, 8):
        for n_blocks in sorted({0, nd - 1, nd, nd + 1, 2 * nd + 3, 29}):
            for name, desc in shard_scenarios(n_blocks).items():
                cases.append((f"{name}-nd{nd}-b{n_blocks}", nd, n_blocks, desc))
    return cases


def test_shard_layout_and_stats_are_what_the_three_sites_computed(driver, tmp_path):
    cases = shard_cases()
    ans = run_driver(driver, tmp_path, [[0, nd] + desc_words(desc) for _, nd, _, desc in cases])
    took, block_counts, uniformity = set(), set(), set()
    for name, nd, n_blocks, desc in cases:
        block_counts.add("below" if n_blocks < nd else "equal" if n_blocks == nd else "above")
        for di in range(nd):
            n_local, n_words, dd, stats = arena_load_shard_before(desc, n_blocks, di, nd, took)
            assert (n_local, n_words, dd, stats) == plan_arena_shard_before(desc, n_blocks, di, nd)[:3] + (stats,), name
            _, _, _, dst_off, stats_plan = plan_arena_shard_before(desc, n_blocks, di, nd)
            assert stats_plan == stats, name
            assert ans.take(2) == [n_local, n_words], (name, di)
            got = [ans.take(3) for _ in range(n_local * 3)]
            assert got == dd, (name, di)
            spans = [ans.take(2) for _ in range(n_local)]
            assert [s[0] for s in spans] == dst_off, (name, di)
            assert [s[1] for s in spans] == [block_span_words_before(dd[lb * 3: lb * 3 + 3]) for lb in range(n_local)], (name, di)
            want = stats["sum_words"] + stats["max_staged_words"] + stats["fixed_m"] + stats["fixed_k"] + stats["geometry_uniform"]
            assert ans.take(15) == want, (name, di)
            assert ans.take(15) == want, (name, di, "the fold alone, as stream_finish runs it")
            for c in range(3):
                if n_local:
                    uniformity.add("uniform" if stats["geometry_uniform"][c] else "mixed")
            if any(all(m == 0 for _, m, _ in dd[lb * 3: lb * 3 + 3]) for lb in range(n_local)):
                took.add("block-of-nil-filters")
            if n_local and any(dd[c][1] == 0 and stats["fixed_m"][c] for c in range(3)):
                took.add("first-of-kind-nil")
            for edge in (1023, 1024, 1025):                    # just under, at and just over a multiple of 1 024 bits = one alignment unit
                if any(m == edge for _, m, _ in got):
                    took.add("m-%d" % edge)
            if any(m == CAP_BITS for _, m, _ in dd):
                took.add("exactly-lds-cap")
            if any(m == CAP_BITS + 1 for _, m, _ in dd):
                took.add("one-word-over-lds-cap")
            # what the probe side and fill_arena rely on: 128-byte alignment, no overlap, everything inside the shard before its pad
            placed = sorted((off, (m + 63) // 64) for off, m, _ in got if m)
            assert all(off % K_ALIGN_WORDS == 0 for off, _ in placed), (name, di)
            assert all(a[0] + a[1] <= b[0] for a, b in zip(placed, placed[1:])), (name, di)
            assert not placed or placed[-1][0] + placed[-1][1] <= n_words - K_ALIGN_WORDS, (name, di)
    assert ans.done()
    assert took == {"nil", "stageable", "beyond-lds", "adopt", "mismatch-m", "mismatch-k", "match", "block-of-nil-filters", "first-of-kind-nil",
                    "exactly-lds-cap", "one-word-over-lds-cap", "m-1023", "m-1024", "m-1025"}, took
    assert [block_span_words_before([(0, m, 1)]) for m in (1023, 1024, 1025)] == [16, 16, 32]
    assert block_counts == {"below", "equal", "above"} and uniformity == {"uniform", "mixed"}
    # a filter of exactly kLdsCapWords words is staged by a probe, one a word larger is not
    s = new_stats()
    fold_before(s, 0, CAP_BITS, 1, set())
    fold_before(s, 1, CAP_BITS + 1, 1, set())
    assert s["max_staged_words"][:2] == [K_LDS_CAP_WORDS, 0]


# ---- parts ----

def packed(ms, gap_before=0, gaps=None, k=7):
    """descriptors laid out in index order; gaps[i]: words left free in front of filter i"""
    desc, at = [], gap_before
    for i, m in enumerate(ms):
        at += (gaps or {}).get(i, 0)
        desc.append((at if m else 0, m, k))
        at += (m + 63) // 64
    return desc, at


def parts_cases():
    """(name, desc, n_words, sections, ranges, region_cap)"""
    out = []
    ms = [1000, 64, 0, 5000, 0, 0, 0, 0, 0, 130, 77, 1 << 20, 0, 9, 640]                     # 15 filters = 5 blocks; block 2 and filter run [4, 9) all nil
    tight, n_tight = packed(ms)
    gappy, n_gappy = packed(ms, gap_before=5, gaps={3: 7, 9: 40, 13: 3})
    for name, desc, nw in (("tight", tight, n_tight), ("gappy", gappy, n_gappy + 11)):
        for ranges in ([(0, 15)], [(0, 4), (4, 9), (9, 15)], [(0, 3), (3, 15)], [(0, 1), (1, 2), (2, 3), (3, 11), (11, 15)], [(0, 6), (6, 9), (9, 12), (12, 15)]):
            out.append((f"{name}-words-{len(ranges)}", desc, nw, 0, ranges, 0))
            if all(a % 3 == 0 and b % 3 == 0 for a, b in ranges):                              # unit 3: whole blocks
                total = sum(section_len_before(desc[b * 3: b * 3 + 3]) for b in range(5))
                for cap in (total, total - 1, total + 1, 0):
                    out.append((f"{name}-sections-{len(ranges)}-cap{cap - total:+d}", desc, nw, 1, ranges, cap))
    # a layout that does not ascend: the second filter sits in front of the first
    swapped = [(100, 6400, 7), (0, 6400, 7), (200, 64, 7)]
    out.append(("descending-1", swapped, 201, 0, [(0, 3)], 0))
    out.append(("descending-2", swapped, 201, 0, [(0, 1), (1, 3)], 0))
    out.append(("descending-sections", swapped, 201, 1, [(0, 3)], 10 ** 6))
    # ... and one that overlaps without going back below the predecessor's start
    out.append(("overlapping", [(0, 6400, 7), (50, 6400, 7)], 150, 0, [(0, 1), (1, 2)], 0))
    out.append(("nothing-present", [(0, 0, 0)] * 6, 4, 0, [(0, 3), (3, 6)], 0))
    rng = np.random.default_rng(7)
    for n in range(40):
        nf = 3 * int(rng.integers(1, 12))
        ms_r = [int(rng.choice([0, int(rng.integers(1, 20000))])) for _ in range(nf)]
        desc, nw = packed(ms_r, gap_before=int(rng.integers(0, 3)), gaps={int(i): int(rng.integers(1, 9)) for i in rng.integers(0, nf, 3)})
        unit = (1, 3)[n % 2]
        cuts = sorted({0, nf} | {int(c) // unit * unit for c in rng.integers(0, nf + 1, int(rng.integers(0, 4)))})
        ranges = list(zip(cuts, cuts[1:]))
        out.append((f"random-{n}-unit{unit}", desc, nw + int(rng.integers(0, 5)), int(unit == 3), ranges, 10 ** 9))
    return out


def test_parts_are_what_the_two_routes_planned(driver, tmp_path):
    cases = parts_cases()
    local_of = {}
    inputs = []
    for name, desc, n_words, sections, ranges, cap in cases:
        words = [1] + desc_words(desc) + [n_words, sections, len(ranges)] + [x for r in ranges for x in r] + [cap, POISON]
        if sections:                                                                           # a part's own offsets: its sections back to back
            local_of[name] = []
            for i0, i1 in ranges:
                loc = [0]
                for b in range(i0 // 3, i1 // 3):
                    loc.append(loc[-1] + section_len_before(desc[b * 3: b * 3 + 3]))
                local_of[name].append(loc)
                words += loc
        inputs.append(words)
    ans = run_driver(driver, tmp_path, inputs)
    took = set()
    for name, desc, n_words, sections, ranges, cap in cases:
        want, total = entries_parts_before(desc, ranges, n_words, sections, took)
        ascending = ascending_before(desc)
        took.add("ascending" if ascending else "not-ascending")
        took.add("unit-3" if sections else "unit-1")
        assert ans.take(3) == [int(ascending), total, int(total <= cap)], name
        if sections:
            took.add("cap-met" if total == cap else "cap-one-short" if total == cap + 1 else "cap-other")
        got = [tuple(ans.take(4)) for _ in ranges]
        assert got == want, name
        t_want, t_total = tables_parts_before(desc, ranges, n_words, sections)
        assert t_total == total and [g[2:] for g in got] == [t[2:] for t in t_want], name
        if not sections:
            assert [g[:2] for g in got] == [t[:2] for t in t_want], name
            buf = np.full(n_words, POISON, dtype="<u8")
            zero_fill_before(buf, n_words, want, took)
            assert ans.take(n_words) == [int(x) for x in buf], name
            if ascending:                     # (the callers cut a layout that does not ascend into one part, or refuse it)
                # exactly the words some part owns are left alone
                owned = np.zeros(n_words, dtype=bool)
                for lo, hi, _, _ in got:
                    owned[lo:hi] = True
                assert np.array_equal(buf == POISON, owned), name
                spans = sorted((lo, hi) for lo, hi, _, _ in got if hi > lo)
                assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), name
        else:
            sec_off = [POISON] * (len(desc) // 3 + 1)
            scatter_before(sec_off, ranges, want, local_of[name])
            assert ans.take(len(sec_off)) == sec_off, name
            # the regions tile [0, total) in part order, and the offsets are the sections back to back
            at = 0
            for _, _, off, length in got:
                assert off == at, name
                at += length
            assert at == total, name
            if ranges[0][0] == 0 and ranges[-1][1] == len(desc):
                lens = [section_len_before(desc[b * 3: b * 3 + 3]) for b in range(len(desc) // 3)]
                assert sec_off == [sum(lens[:b]) for b in range(len(lens) + 1)], name
    assert ans.done()
    assert took == {"part-of-nil-filters", "single-part", "ascending", "not-ascending", "unit-1", "unit-3", "cap-met", "cap-one-short", "cap-other",
                    "gap-before", "gap-between", "gap-behind"}, took


# ---- the route of one filter ----

def route_cases():
    """(m, n_entries, k, bin_min_locs, bin_scratch_bytes)"""
    big = CAP_BITS + 64 * 1024                                    # beyond LDS under either head
    out = []
    for head in (0, K_SET_LIST_BYTES):                            # the LDS boundary of both routes, bit by bit around the last word
        edge = (K_LDS_BUDGET - head) // 8 * 64
        for m in (edge - 64, edge - 1, edge, edge + 1, edge + 64, edge + 65):
            out.append((m, 1 << 20, 10, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
            out.append((m, 10, 1, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
    for m in ((1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 33):
        out.append((m, 1 << 20, 10, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
    for n_locs in (BIN_MIN_LOCS - 1, BIN_MIN_LOCS, BIN_MIN_LOCS + 1):
        out.append((big, n_locs, 1, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
    out += [(big, 0, 7, 0, K_BIN_SCRATCH_BYTES), (big, 1, 1, 0, K_BIN_SCRATCH_BYTES), (big, 1, 1, 1, K_BIN_SCRATCH_BYTES)]     # lab key 6 at 0: one location is enough
    for n_locs in ((1 << 32) - 4097, (1 << 32) - 4096, (1 << 32) - 4095):
        out.append((big, n_locs, 1, BIN_MIN_LOCS, 1 << 40))
        out.append((big, n_locs // 7 + 1, 7, BIN_MIN_LOCS, 1 << 40))
    for scratch in (4 * (5 << 20) - 1, 4 * (5 << 20), 4 * (5 << 20) + 1, 0):                   # 0: lab key 2
        out.append((big, 5 << 20, 1, BIN_MIN_LOCS, scratch))
        out.append((big, 1 << 20, 5, BIN_MIN_LOCS, scratch))
    return out


def test_route_choice_is_what_each_build_route_decided(driver, tmp_path):
    cases = route_cases()
    inputs = [[2, m, n, k, head, lo, scratch] for m, n, k, lo, scratch in cases for head in (0, K_SET_LIST_BYTES)]
    ans = run_driver(driver, tmp_path, inputs)
    took, routes = set(), {0: set(), K_SET_LIST_BYTES: set()}
    differ = 0
    for m, n, k, lo, scratch in cases:
        want_entries = entries_route_before(m, n, k, lo, scratch, took)
        want_tables = tables_route_before(m, n, k, lo, scratch, took)
        assert ans.take() == want_entries, (m, n, k, lo, scratch, "entries route: head 0")
        assert ans.take() == want_tables, (m, n, k, lo, scratch, "tables route: head kSetListBytes")
        routes[0].add(want_entries)
        routes[K_SET_LIST_BYTES].add(want_tables)
        differ += want_entries != want_tables
        if scratch == 0 and (m + 63) // 64 > K_LDS_CAP_WORDS:
            assert want_entries == want_tables == SLICED
    assert ans.done()
    assert routes[0] == routes[K_SET_LIST_BYTES] == {STAGED, BINNED, SLICED}
    assert differ > 0                                             # the two heads are two thresholds
    assert took == {"not:m-below-2^31", "not:enough-locs", "not:locs-below-2^32-4096", "not:locs-fit-scratch"}, took
    # each condition of binned_build_fits flips at its edge, the others held
    flips = lambda a, b: entries_route_before(*a, set()) != entries_route_before(*b, set())
    big = CAP_BITS + 64 * 1024
    assert flips(((1 << 31) - 1, 1 << 20, 10, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES), (1 << 31, 1 << 20, 10, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
    assert flips((big, BIN_MIN_LOCS - 1, 1, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES), (big, BIN_MIN_LOCS, 1, BIN_MIN_LOCS, K_BIN_SCRATCH_BYTES))
    assert flips((big, (1 << 32) - 4097, 1, BIN_MIN_LOCS, 1 << 40), (big, (1 << 32) - 4096, 1, BIN_MIN_LOCS, 1 << 40))
    assert flips((big, 5 << 20, 1, BIN_MIN_LOCS, 4 * (5 << 20)), (big, 5 << 20, 1, BIN_MIN_LOCS, 4 * (5 << 20) - 1))


# ---- balanced cuts ----

def cuts_cases():
    rng = np.random.default_rng(3)
    out = []
    for cost in ([], [5], [0, 0, 0, 0], [1] * 9, [100, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 100], [0, 0, 50, 0, 0, 50, 0, 0, 0], [7] * 24):
        for parts in (1, 2, 3, 8, 50):
            for unit in (1, 3):
                out.append((parts, unit, cost))
    for _ in range(60):
        n = int(rng.integers(1, 200))
        cost = [int(x) for x in rng.integers(0, 10 ** int(rng.integers(1, 10)), n)]
        out.append((int(rng.integers(1, 10)), (1, 3)[int(rng.integers(0, 2))], cost))
    return out


def test_balanced_cuts_are_the_parents(driver, tmp_path):
    cases = cuts_cases()
    ans = run_driver(driver, tmp_path, [[3, parts, unit, len(cost)] + cost for parts, unit, cost in cases])
    fewer, full = 0, 0
    for parts, unit, cost in cases:
        want = balanced_cuts_before(cost, parts, unit)
        got = ans.take(ans.take())
        assert got == want, (parts, unit, cost)
        # what the callers rely on: boundaries from 0 to n, at most `parts` runs, cut on whole units; no run is empty unless there is nothing to cut
        assert got[0] == 0 and got[-1] == len(cost) and len(got) - 1 <= max(parts, 1)
        assert all(c % unit == 0 for c in got[1:-1])
        assert all(a < b for a, b in zip(got, got[1:])) or len(cost) == 0
        fewer += len(got) - 1 < parts
        full += len(got) - 1 == parts
    assert ans.done() and fewer and full
