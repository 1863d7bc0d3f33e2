"""The device ingest's plan on the host (no GPU): tests/ingest_plan_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/ingest_plan.hpp — the arithmetic ingest_api.inc lays its distinct-entry tables out by, sizes and grows them
by, deals rows to waves by, partitions the file-level union by, picks a walker by and checks its row arguments by.  The program is
built twice, with -Wall -Wextra -Werror and under the address and undefined-behaviour sanitizers, and run directly.

Reference: the arithmetic that header replaced, restated below site by site from ingest_api.inc and match_api.inc as they stood at
commit 4225d42 (the line numbers are those files'), when every site wrote its own copy.  On top of the comparison, what the kernels
and the callers rely on is asserted by itself: tables of one block do not overlap, the fingerprints sit total_slots * 4 words behind
the block's start, a block is total_slots * 40 bytes, a wave's run is a multiple of 64 rows, the waves cover the rows and none is
empty."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bloomsearch_amd", "csrc")
U32 = 0xFFFFFFFF
FAULTS = ("none", "offsets-not-monotone", "bytes-missing", "set-first-span", "set-first-not-monotone", "parents-missing", "parent-out-of-range")


def constant(header, pattern):
    found = re.search(pattern, open(os.path.join(CSRC, header)).read(), flags=re.M)
    assert found, (header, pattern)
    return int(found.group(1))


PART_TARGET = constant("ingest.hip.h", r"constexpr uint32_t kPartTarget = (\d+);")
INGEST_WPE = constant("ingest.hip.h", r"#define BSG_INGEST_WPE (\d+)$")
THREADS = {"walkers": constant("ingest.hip.h", r"constexpr int kIngestThreads = (\d+);"),
           "minmax": constant("minmax.hip.h", r"constexpr int kMinMaxThreads = (\d+);"),
           "buckets": constant("hist.hip.h", r"constexpr int kBucketThreads = (\d+);")}


# ---- the parent's arithmetic, site by site ----

def pow2_at_least_before(n):
    """ingest_api.inc:162-167"""
    c = 64
    while c < n and c < (1 << 31):
        c <<= 1
    return c


def shift_for_before(cap):
    """ingest_api.inc:169-174"""
    lg = 0
    while (1 << lg) < cap:
        lg += 1
    return 32 - lg


def make_table_before(first_slot, total_slots, cap):
    """ingest_api.inc:176-179: (slots, fps) in 8-byte words from the block's base, mask, shift"""
    return (first_slot * 4, total_slots * 4 + first_slot, cap - 1, shift_for_before(cap))


def run_layout_before(caps):
    """the running first_slot of ingest_api.inc:452-470, 558-572, 756-771 and 921-935: (total, [make_table of every table])"""
    first, total = [], 0
    for cap in caps:
        first.append(total)
        total += cap
    return total, [make_table_before(f, total, c) for f, c in zip(first, caps)]


def oneshot_want_before(kind, rows_in, hint):
    """ingest_api.inc:457-459 (ingest_rows_part)"""
    want = 256 if kind == 0 else max(1024, rows_in * 4)
    if hint:
        want = hint
    return want


def stream_want_before(kind, hint):
    """ingest_api.inc:911 and 925-927 (stream_add_sets)"""
    want = 256 if kind == 0 else 1024
    if hint:
        want = hint
    return want


def parent_want_before(child_sum):
    """ingest_api.inc:562 (union_global_tables) and 763 (merge_parents)"""
    return max(64, child_sum * 2)


def grown_before(cap):
    """ingest_api.inc:207-208 (grow_overflowed): None = refused"""
    cap *= 4
    return None if cap > (1 << 31) else cap


def descriptor_room_before(nt):
    """ingest_api.inc:939 (stream_add_sets), in 32-bit arithmetic"""
    return max(96, nt if nt > 0x7FFFFFFF else (nt * 2) & U32)


def minmax_room_before(n_sets, roomy, nf):
    """ingest_api.inc:356-357 (minmax_reserve): None = refused"""
    room = max(32, n_sets * 2) if roomy else max(n_sets, 1)
    return None if room * nf > 0x7FFFFFFF else room


def wave_runs_before(n, n_cus, wps, threads):
    """ingest_api.inc:308-312 (walk_chunks, wps = BSG_INGEST_WPE), 400-404 (MinMaxWalk::launch, 8) and match_api.inc:569-573 (8)"""
    max_waves = n_cus * 4 * wps
    waves = min((n + 63) // 64, max_waves)
    rows_per_wave = (((n + waves - 1) // waves + 63) // 64 * 64) & U32
    used, wpw = (n + rows_per_wave - 1) // rows_per_wave, threads // 64
    return rows_per_wave, ((used + wpw - 1) // wpw) & U32


def first_log2p_before(child_sum, coarsen):
    """ingest_api.inc:619-622 (union_partitioned)"""
    lg = 0
    while (child_sum >> lg) > PART_TARGET and lg < 24:
        lg += 1
    if coarsen < 32:
        lg -= min(lg, coarsen)
    else:
        lg = min(lg + (coarsen - 32), 24)
    return lg


def finer_before(lg):
    """ingest_api.inc:659"""
    return min(lg + 2, 26)


def walker_before(by_set, spec, gram):
    """the ladders at ingest_api.inc:515-520 (grouped) and 1261-1266 (by set): the kernel's name"""
    if by_set:
        return "k_ingest_rows_sets_gram" if spec and gram else "k_ingest_rows_sets_tok" if spec else "k_ingest_rows_sets"
    return "k_ingest_rows_gram" if spec and gram else "k_ingest_rows_tok" if spec else "k_ingest_rows"


def check_rows_before(off, have_bytes):
    """ingest_api.inc:844-847, 1431-1433 and 1473-1475"""
    for r in range(len(off) - 1):
        if off[r + 1] < off[r]:
            return "offsets-not-monotone", r
    if off[-1] and not have_bytes:
        return "bytes-missing", 0
    return "none", 0


def check_set_first_before(sfr, n_rows):
    """ingest_api.inc:841-843 (ingest_rows_call)"""
    if sfr[0] != 0 or sfr[-1] != n_rows:
        return "set-first-span", 0
    for s in range(len(sfr) - 1):
        if sfr[s + 1] < sfr[s]:
            return "set-first-not-monotone", s
    return "none", 0


def check_parents_before(parents, n_sets, n_parents):
    """ingest_api.inc:963-969 (check_parents) and, with n_sets > 0, 848-850"""
    if n_sets and n_parents and parents is None:
        return "parents-missing", 0
    for s in range(n_sets if parents is not None else 0):
        if parents[s] != U32 and parents[s] >= n_parents:
            return "parent-out-of-range", s
    return "none", 0


def too_many_before(n):
    """ingest_api.inc:981, 1166, 1405 and 1509"""
    return n > U32 // 3


# ---- the driver ----

@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    out = tmp_path_factory.mktemp("ingest_plan")
    exes = []
    for name, flags in (("plain", ["-O2", "-Wall", "-Wextra", "-Werror"]),
                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = out / ("ingest_plan_check_" + name)
        subprocess.run(["g++", "-std=c++17", *flags, "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "ingest_plan_check.cpp")],
                       check=True, timeout=300)
        exes.append(exe)
    return out, exes


def ask(drivers, commands):
    """every command through both builds: a list of integers per command"""
    out, exes = drivers
    inp = out / "commands.txt"
    inp.write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
    answers = []
    for exe in exes:
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (exe.name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        lines = r.stdout.split("\n")
        assert len(lines) == len(commands) + 1 and lines[-1] == "", exe.name
        answers.append([[int(x) for x in line.split()] for line in lines[:-1]])
    assert answers[0] == answers[1]
    return answers[0]


def check_block(name, total, tables):
    """tables: (cap, first_slot, slots_word, fps_word, mask, shift) of one block"""
    spans = []
    for cap, first, slots, fps, _, _ in tables:
        assert slots == first * 4 and fps - first == total * 4, name          # the fingerprints: total_slots * 4 words behind the block's start
        spans += [(slots, slots + cap * 4), (fps, fps + cap)]
    assert all(b <= total * 4 for a, b in spans[0::2]) and all(a >= total * 4 and b <= total * 5 for a, b in spans[1::2]), name
    spans.sort()
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])), name          # no two tables overlap
    assert sum(t[0] for t in tables) == total, name


HINTS = [0, 1, 64, 65, 1 << 31, (1 << 31) + 1]
ROWS_IN = [0, 255, 256, 257, 1 << 30]


def test_capacities_are_what_every_site_computed(drivers):
    commands, want = [], []
    for n in sorted(set(HINTS + [63, 127, 128, 129, 255, 256, 1 << 30, (1 << 30) + 1, (1 << 32) + 5, 1 << 40])):
        commands.append(("pow2", n))
        want.append([pow2_at_least_before(n), shift_for_before(pow2_at_least_before(n))])
    for kind in range(3):
        for hint in HINTS:
            for rows_in in ROWS_IN:
                w = oneshot_want_before(kind, rows_in, hint)
                commands.append(("oneshot", kind, rows_in, hint))
                want.append([w, pow2_at_least_before(w)])
            w = stream_want_before(kind, hint)
            commands.append(("stream", kind, hint))
            want.append([w, pow2_at_least_before(w)])
    for child_sum in (0, 1, 31, 32, 33, 1000, 1 << 29, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 32, 3 << 32):
        w = parent_want_before(child_sum)
        commands.append(("parent", child_sum))
        want.append([w, pow2_at_least_before(w)])
    got = ask(drivers, commands)
    for c, g, w in zip(commands, got, want):
        assert g == w, c
    by = {c: g for c, g in zip(commands, got)}
    assert by[("pow2", (1 << 31) + 1)] == [1 << 31, 1]                        # clamped to 2^31
    assert by[("oneshot", 1, 1 << 30, 0)] == [1 << 32, 1 << 31]               # 4 x the rows reaches the clamp
    assert by[("oneshot", 0, 1 << 30, 0)] == [256, 256] and by[("oneshot", 2, 255, 0)] == [1024, 1024] and by[("oneshot", 2, 257, 0)] == [1028, 2048]
    assert by[("oneshot", 1, 257, 65)] == [65, 128] and by[("stream", 0, 0)] == [256, 256] and by[("stream", 2, 0)] == [1024, 1024]
    assert by[("parent", 0)] == [64, 64] and by[("parent", 33)] == [66, 128]


def test_growth_room_and_refusals(drivers):
    commands, want = [], []
    for cap in (64, 256, 1 << 28, 1 << 29, 1 << 30, 1 << 31):
        commands.append(("grow", cap))
        want.append([grown_before(cap) or 0])
    for sets in (0, 32, 33, 48):
        for parents in (0, 2):
            nt = (sets + parents) * 3
            commands.append(("room", nt))
            want.append([descriptor_room_before(nt)])
    for nt in (47, 48, 49, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, U32 // 3 * 3):
        commands.append(("room", nt))
        want.append([descriptor_room_before(nt)])
    for nf in (1, 8):
        bound = 0x7FFFFFFF // nf
        for roomy in (0, 1):
            for sets in (0, 1, 16, 17, 32, 33, 48, bound // 2, bound // 2 + 1, bound, bound + 1, U32):
                commands.append(("mmroom", sets, roomy, nf))
                want.append([minmax_room_before(sets, roomy, nf) or 0])
    got = ask(drivers, commands)
    for c, g, w in zip(commands, got, want):
        assert g == w, c
    by = {c: g[0] for c, g in zip(commands, got)}
    assert by[("grow", 1 << 29)] == 1 << 31 and by[("grow", 1 << 30)] == 0 and by[("grow", 64)] == 256
    assert by[("room", 0)] == 96 and by[("room", 48)] == 96 and by[("room", 49)] == 98 and by[("room", 0x80000000)] == 0x80000000
    assert by[("mmroom", 0, 0, 1)] == 1 and by[("mmroom", 0, 1, 1)] == 32 and by[("mmroom", 16, 1, 8)] == 32 and by[("mmroom", 17, 1, 8)] == 34
    assert by[("mmroom", 0x7FFFFFFF, 0, 1)] == 0x7FFFFFFF and by[("mmroom", 0x80000000, 0, 1)] == 0
    assert by[("mmroom", 0x0FFFFFFF, 0, 8)] == 0x0FFFFFFF and by[("mmroom", 0x10000000, 0, 8)] == 0
    assert by[("mmroom", 0x7FFFFFFF // 2, 1, 1)] == 0x7FFFFFFE and by[("mmroom", 0x7FFFFFFF // 2 + 1, 1, 1)] == 0


def test_layouts_of_sets_and_parents(drivers):
    commands, want = [], []
    for n_sets in (1, 2, 33):
        rows_in = [(s * 37) % 700 for s in range(n_sets)]
        hints = [(0, 65 if s % 2 else 0, 1 if s % 3 == 0 else 0) for s in range(n_sets)]
        oneshot = [oneshot_want_before(k, rows_in[s], hints[s][k]) for s in range(n_sets) for k in range(3)]
        stream = [stream_want_before(k, hints[s][k]) for s in range(n_sets) for k in range(3)]
        for name, wants in (("oneshot", oneshot), ("stream", stream)):
            commands.append(("layout", 0, len(wants), *wants))
            want.append(("%s-%d" % (name, n_sets), False, wants))
        for n_parents in (0, 2):
            # the children's exact counts, as finish_part sums them per parent table: one parent takes every third set
            sums = [sum((s + 1) * (k + 2) * 11 for s in range(n_sets) if s % 3 == p % 3) for p in range(n_parents) for k in range(3)]
            commands.append(("layout", 0, len(sums), *[parent_want_before(x) for x in sums]))       # union_global_tables / merge_parents
            want.append(("parents-%d-%d" % (n_sets, n_parents), False, [parent_want_before(x) for x in sums]))
            commands.append(("layout", 1, len(sums), *sums))                                        # union_partitioned: dense, a slot per child entry
            want.append(("dense-%d-%d" % (n_sets, n_parents), True, sums))
    commands.append(("layout", 0, 1, 64))                                                           # the parents' placeholder (ingest_api.inc:473-478, 998-1003)
    want.append(("placeholder", False, [64]))
    commands.append(("layout", 0, 1, 1024))                                                         # a grown table, alone in its block (ingest_api.inc:210-213)
    want.append(("grown", False, [1024]))
    got = ask(drivers, commands)
    for (name, dense, wants), g in zip(want, got):
        total, n_bytes, flat = g[0], g[1], g[2:]
        tables = [tuple(flat[i: i + 6]) for i in range(0, len(flat), 6)]
        assert len(tables) == len(wants) and n_bytes == total * 40, name
        if dense:
            # ingest_api.inc:603 and 612-613: first[t] runs over the sums themselves; the list's own mask and shift at 665
            first, run = [], 0
            for x in wants:
                first.append(run)
                run += x
            assert total == run, name
            for t, (x, f) in zip(tables, zip(wants, first)):
                assert t == (x, f, f * 4, run * 4 + f, (x - 1) & U32, 0), name
        else:
            caps = [pow2_at_least_before(x) for x in wants]
            total_before, made = run_layout_before(caps)
            assert total == total_before, name
            assert [t[2:] for t in tables] == made and [t[0] for t in tables] == caps, name
        check_block(name, total, tables)
    by = {w[0]: g for w, g in zip(want, got)}
    assert by["placeholder"] == [64, 2560, 64, 0, 0, 256, 63, 26]                                   # make_table(ph, 0, 64, 64)
    assert by["oneshot-1"][0] == 256 + 1024 + 64                                                    # hint 1 -> 64 slots
    # a dense list of n entries inside a block (ingest_api.inc:665) and alone in its own (merge_parents, 790)
    got = ask(drivers, [("place", 10, 100, 7, 1), ("place", 0, 7, 7, 1), ("place", 64, 192, 128, 0)])
    assert got == [[40, 410, 6, 0], [0, 28, 6, 0], list(make_table_before(64, 192, 128))]


def test_rows_per_wave_and_grid(drivers):
    commands = []
    for n_cus in (1, 256):
        for wps in sorted({INGEST_WPE, 8}):
            for threads in sorted(set(THREADS.values())):
                W = n_cus * 4 * wps
                for n in (1, 63, 64, 65, 64 * W, 64 * W + 1, 64 * W * 3 - 1, (1 << 32) - 1):
                    commands.append(("wave", n, n_cus, wps, threads))
    assert INGEST_WPE != 8 and set(THREADS.values()) <= {64, 128, 256, 512, 1024}
    got = ask(drivers, commands)
    for (_, n, n_cus, wps, threads), (rpw, grid) in zip(commands, got):
        case = (n, n_cus, wps, threads)
        assert (rpw, grid) == wave_runs_before(n, n_cus, wps, threads), case
        used = (n + rpw - 1) // rpw
        assert rpw % 64 == 0 and rpw > 0, case
        assert used <= n_cus * 4 * wps and used * rpw >= n, case               # the waves used cover n
        assert (used - 1) * rpw < n, case                                      # the last wave is not empty
        assert grid == -(-used // (threads // 64)), case                       # waves used / waves per workgroup, rounded up


def test_partition_fineness(drivers):
    sums = [0, 1, PART_TARGET, PART_TARGET + 1, 2 * PART_TARGET, 2 * PART_TARGET + 1, PART_TARGET << 23, (PART_TARGET << 23) + 1,
            PART_TARGET << 24, (PART_TARGET << 24) + 1, PART_TARGET << 30, (1 << 64) - 1]
    coarsens = [0, 1, 31, 32, 34, 56]
    commands = [("log2p", s, PART_TARGET, c) for s in sums for c in coarsens] + [("finer", lg) for lg in range(0, 28)]
    got = ask(drivers, commands)
    for c, (g,) in zip(commands, got):
        assert g == (first_log2p_before(c[1], c[3]) if c[0] == "log2p" else finer_before(c[1])), c
    by = {c: g[0] for c, g in zip(commands, got)}
    assert by[("log2p", PART_TARGET, PART_TARGET, 0)] == 0 and by[("log2p", PART_TARGET + 1, PART_TARGET, 0)] == 1
    assert by[("log2p", PART_TARGET << 24, PART_TARGET, 0)] == 24 and by[("log2p", (PART_TARGET << 24) + 1, PART_TARGET, 0)] == 24
    assert by[("log2p", PART_TARGET << 30, PART_TARGET, 31)] == 0 and by[("log2p", PART_TARGET << 30, PART_TARGET, 34)] == 24
    assert by[("log2p", 0, PART_TARGET, 34)] == 2 and by[("log2p", 0, PART_TARGET, 56)] == 24
    for start in (0, 21, 22, 24):                                              # three retries in a row
        lg, steps = start, []
        for _ in range(3):
            lg = by[("finer", lg)]
            steps.append(lg)
        assert steps == [min(start + 2, 26), min(start + 4, 26), min(start + 6, 26)]


def test_every_walker_has_one_slot_and_the_table_lists_it_there(drivers):
    cells = [(by_set, spec, gram) for by_set in (0, 1) for spec, gram in ((0, 0), (1, 0), (1, 1))]
    got = [g[0] for g in ask(drivers, [("slot", *c) for c in cells])]
    assert sorted(got) == list(range(6))                                       # all six, each hit once
    api = open(os.path.join(CSRC, "ingest_api.inc")).read()
    table = api[api.index("kIngestWalkers[bsh::kWalkerSlots]"): api.index("void launch_walker(")]
    kernels = re.findall(r"walker\(c, bsg::(\w+),", table)
    assert len(kernels) == 6
    for cell, slot in zip(cells, got):
        assert kernels[slot] == walker_before(*cell), cell
    # a default tokenizer's width is never read (the ladders tested the spec first)
    assert ask(drivers, [("slot", 0, 0, 1), ("slot", 1, 0, 1)]) == [[0], [3]]
    for k in kernels:
        assert api.count("bsg::%s," % k) == 1, k                               # launched from the table alone


def test_row_argument_checks_name_the_first_fault(drivers):
    commands, want = [], []

    def rows(off, have_bytes):
        commands.append(("rows", len(off) - 1, have_bytes, *off))
        want.append(check_rows_before(off, have_bytes))

    def set_first(sfr, n_rows):
        commands.append(("setfirst", len(sfr) - 1, n_rows, *sfr))
        want.append(check_set_first_before(sfr, n_rows))

    def parents(p, n_sets, n_parents):
        commands.append(("parents", n_sets, n_parents, int(p is not None), *(p or [])))
        want.append(check_parents_before(p, n_sets, n_parents))

    rows([0], 0)
    rows([7], 0)                                   # bytes before the first row count as bytes
    rows([0, 0, 0], 0)
    rows([0, 5, 9], 1)
    rows([0, 5, 9], 0)
    rows([0, 5, 4, 3, 9], 1)                       # two faults: the first is named
    rows([3, 2], 0)                                # not monotone is found before the missing bytes
    rows([0, 1 << 40, (1 << 40) - 1], 1)
    set_first([0, 0], 0)
    set_first([0, 4, 9], 9)
    set_first([1, 4, 9], 9)
    set_first([0, 4, 8], 9)
    set_first([0, 6, 5, 4, 9], 9)
    set_first([0, 9, 3, 9], 9)
    set_first([1, 0, 9], 9)                        # the span is checked before the order
    parents(None, 0, 2)
    parents(None, 3, 0)
    parents(None, 3, 2)
    parents([0, 1, U32], 3, 2)
    parents([0, 2, 3], 3, 2)
    parents([U32, U32, 7], 3, 0)
    parents([5], 1, 5)
    parents([4], 1, 5)
    for n in (0, U32 // 3, U32 // 3 + 1, 1 << 33):
        commands.append(("toomany", n))
        want.append(int(too_many_before(n)))
    got = ask(drivers, commands)
    for c, g, w in zip(commands, got, want):
        if c[0] == "toomany":
            assert g == [w], c
        else:
            assert (FAULTS[g[0]], g[1]) == w, c
    assert want[5] == ("offsets-not-monotone", 1) and want[6] == ("offsets-not-monotone", 0) and want[4] == ("bytes-missing", 0)
    assert want[12] == ("set-first-not-monotone", 1) and want[14] == ("set-first-span", 0)
    assert want[17] == ("parents-missing", 0) and want[19] == ("parent-out-of-range", 1) and want[20] == ("parent-out-of-range", 2)


def test_the_entry_points_keep_their_words():
    """the messages the answers of the checks are turned into, byte for byte those of the parent"""
    api = open(os.path.join(CSRC, "ingest_api.inc")).read()
    for text in ('"row_off not monotone at %u"', '"rows is null"', '"set_first_row must span [0, n_rows]"', '"set_first_row not monotone at %u"',
                 '"parent_of_set is null"', '"parent_of_set[%u] out of range"', '"too many sets and parents"',
                 '"distinct-entry table %u would exceed 2^31 slots"', '"minmax: too many sets"'):
        assert api.count(text) == 1, text
    plan = open(os.path.join(CSRC, "host", "ingest_plan.hpp")).read()
    assert "#include <hip" not in plan and "hipError_t" not in plan and "namespace bsh {" in plan    # no device type
    assert re.search(r"constexpr uint64_t kSlotBytes = 40;", plan) and "kSlotBytes = " not in api
