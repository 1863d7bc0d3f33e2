"""The arithmetic of a probe call on the host (no GPU): tests/probe_plan_check.cpp, built with plain g++ against
bloomsearch_amd/csrc/host/probe_plan.hpp — the code probe_arenas and query_solo (probe_api.inc) cut a device's shards into launch
groups by, place the survivors by, lay survivor rows out by and merge the per-device bitsets by.  Reference for every comparison:
the loops that header replaced, restated below from bloomsearch_amd/csrc/probe_api.inc as it stood at commit c700865 (the line
numbers are that file's), when probe_arenas still did all of it in one body; for the interleave, its definition ("local bit l of
device di is global bit l * nd + di") in numpy.  On top of the comparison, what the callers rely on is asserted by itself: every
non-empty shard is in exactly one group, in list order; a tail-split cut leaves both parts non-empty."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX_GROUP_ARENAS = 128                                     # kernels.hip.h: what one launch's kernel arguments hold
DEFAULT_BUDGET = 256 << 20                                   # probe_api.inc:305 kGroupScratchBudget
SMALL_BUDGET = 64 << 10
LIMITS = [1, 3, 32, 128, 1024]
N_QUERIES = [1, 256, 4096]
WT = [0, 1, 5]


# ---- the parent's loops, restated ----

def group_add_before(g, n_queries, Wt, n_blocks, idx):
    """probe_api.inc:327-337 (group_add)"""
    G = (n_blocks + 63) // 64
    g["index"].append(idx)
    g["v_words"] += G * max(Wt, 1) * 64
    g["out_words"] += n_queries * G
    g["max_blocks"] = max(g["max_blocks"], n_blocks)
    g["max_G"] = max(g["max_G"], G)
    g["total_G"] += G


def new_group():
    return {"index": [], "v_words": 0, "out_words": 0, "max_blocks": 0, "max_G": 0, "total_G": 0}


def groups_before(local, n_queries, Wt, limit, budget, closed_on=None):
    """probe_api.inc:816-827 (the group cut inside probe_arenas); closed_on collects why a group closed"""
    groups = []
    for i, nb in enumerate(local):
        if nb == 0:
            continue
        G_add = (nb + 63) // 64
        over_out = bool(groups) and (groups[-1]["out_words"] + n_queries * G_add) * 8 > budget
        over_v = bool(groups) and (groups[-1]["v_words"] + G_add * max(Wt, 1) * 64) * 8 > budget
        full = bool(groups) and bool(groups[-1]["index"]) and (over_out or over_v)
        if not groups or len(groups[-1]["index"]) >= limit or full:
            if closed_on is not None and groups:
                closed_on.add("count" if len(groups[-1]["index"]) >= limit else "survivors" if over_out else "verdicts")
            groups.append(new_group())
        group_add_before(groups[-1], n_queries, Wt, nb, i)
    return groups


def out_off_before(global_blocks, n_queries):
    """probe_api.inc:786-788 (out_off; again as aoff at 682-683 and in query_solo at 1425-1426)"""
    off = [0]
    for nb in global_blocks:
        off.append(off[-1] + n_queries * ((nb + 63) // 64))
    return off


def goff_before(groups, out_off, several):
    """probe_api.inc:830-842 (goff: running sum in the device's part buffer, or out_off of the group's first arena)"""
    goff = [0] * (len(groups) + 1)
    if several:
        total = 0
        for gi, g in enumerate(groups):
            goff[gi] = total
            total += g["out_words"]
        goff[len(groups)] = total
    else:
        for gi, g in enumerate(groups):
            goff[gi] = out_off[g["index"][0]]
    return goff


def n0_before(n_shards, pct):
    """probe_api.inc:938-941 (the tail split: its size conditions and the n0 rule); 0 = no cut"""
    if not (pct and n_shards >= 8 and n_shards <= K_MAX_GROUP_ARENAS):
        return 0
    return min(n_shards - 1, max(1, n_shards * pct // 100))


def rows_layout_before(local, n_queries):
    """probe_api.inc:709-724 (rows_layout); local[d][i] = arenas[i]->shards[d].n_blocks"""
    row_base, arena_off = [0], []
    for d in range(len(local)):
        o, offs = 0, []
        for nb in local[d]:
            offs.append(o)
            o += n_queries * ((nb + 63) // 64)
        arena_off.append(offs)
        row_base.append(row_base[-1] + o)
    return row_base, arena_off


def shard_blocks(n_blocks, di, nd):
    """bsg_arena_load: device di holds the global blocks di, di + nd, ..."""
    return (n_blocks - di + nd - 1) // nd if n_blocks > di else 0


# ---- the driver ----

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("probe_plan") / "probe_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "probe_plan_check.cpp")], check=True, timeout=300)
    return exe


class Answers:
    def __init__(self, words):
        self.w, self.at = words, 0

    def take(self, n=None):
        if n is None:
            self.at += 1
            return int(self.w[self.at - 1])
        self.at += n
        return self.w[self.at - n: self.at]


def run_driver(exe, tmp_path, cases):
    """cases: lists / arrays of u64 words, each starting with its kind"""
    words = np.concatenate([np.asarray([len(cases)], dtype="<u8")] + [np.asarray(c, dtype="<u8") for c in cases])
    words.tofile(tmp_path / "cases.bin")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return Answers(np.fromfile(tmp_path / "answers.bin", dtype="<u8"))


def has_bmi2(exe):
    return subprocess.run([str(exe), "bmi2"], capture_output=True, text=True, timeout=60, check=True).stdout.strip() == "1"


# ---- groups and offsets ----

def arena_lists():
    rng = np.random.default_rng(20261016)
    few = [0, 0, 5, 1000, 0, 130, 7, 1, 2, 0, 0, 64, 65, 63, 999, 3, 10001, 0]            # empty arenas first, in the middle, last
    mixed = [int(x) for x in rng.integers(0, 300, 40)]
    mixed[0] = mixed[17] = mixed[18] = mixed[-1] = 0
    many = [int(x) for x in rng.integers(1, 200, 1300)]                                   # beyond every count limit
    for i in (0, 1, 400, 401, 402, 1299):
        many[i] = 0
    return {"few": few, "mixed": mixed, "many": many}


def plan_cases():
    """(name, n_queries, Wt, limit, budget, several, local, global)"""
    out = []
    for name, glob in arena_lists().items():
        for nd in ((1, 3) if name == "many" else (1, 2, 3, 8)):
            for di in range(nd):
                local = [shard_blocks(nb, di, nd) for nb in glob]
                for several in ((0,) if nd == 1 else (0, 1)):                             # (0 on several devices: survivors not wanted on the host)
                    for limit in LIMITS:
                        for nq in N_QUERIES:
                            for Wt in WT:
                                for budget in ((DEFAULT_BUDGET,) if name == "many" else (DEFAULT_BUDGET, SMALL_BUDGET)):
                                    out.append((f"{name}-nd{nd}-di{di}-s{several}-l{limit}-q{nq}-w{Wt}-b{budget}", nq, Wt, limit, budget, several, local, glob))
    return out


def test_groups_and_their_offsets_are_what_probe_arenas_formed(driver, tmp_path):
    cases = plan_cases()
    ans = run_driver(driver, tmp_path, [[0, nq, Wt, limit, budget, several, len(local)] + local + glob
                                        for _, nq, Wt, limit, budget, several, local, glob in cases])
    closed_on, alone_over_budget, device_counts = set(), 0, set()
    for name, nq, Wt, limit, budget, several, local, glob in cases:
        out_off = out_off_before(glob, nq)
        assert [int(x) for x in ans.take(len(glob) + 1)] == out_off, name
        why = set()
        want = groups_before(local, nq, Wt, limit, budget, why)
        got = []
        for _ in range(ans.take()):
            g = new_group()
            g["index"] = [int(x) for x in ans.take(ans.take())]
            for key in ("v_words", "out_words", "max_blocks", "max_G", "total_G"):
                g[key] = ans.take()
            got.append(g)
        assert got == want, name
        assert [int(x) for x in ans.take(len(got) + 1)] == goff_before(want, out_off, several), name
        # by itself: every non-empty shard in exactly one group, in list order; no group beyond the count limit; none empty
        assert [i for g in got for i in g["index"]] == [i for i, nb in enumerate(local) if nb], name
        assert all(1 <= len(g["index"]) <= limit for g in got), name
        for g in got:
            if max(g["out_words"], g["v_words"]) * 8 > budget:
                assert len(g["index"]) == 1, name                  # only a shard that is too large alone exceeds the budget
                alone_over_budget += 1
        if budget == SMALL_BUDGET:
            closed_on |= why
        device_counts.add(name.split("-")[1])
    assert ans.at == len(ans.w)
    # the cases do reach every way a group closes, and a shard larger than the budget
    assert closed_on == {"count", "survivors", "verdicts"} and alone_over_budget > 0
    assert device_counts == {"nd1", "nd2", "nd3", "nd8"}


def test_groups_close_on_survivors_in_one_case_and_on_verdict_words_in_another(driver, tmp_path):
    local = [128] * 40                                                                     # G = 2 each
    # 256 queries: 4 KiB of survivors and 1 KiB of verdict words per shard -> 16 shards fill 64 KiB of survivors
    # 1 query, Wt = 5: 16 bytes of survivors and 5 KiB of verdict words per shard -> 12 shards fit 64 KiB of verdict words
    ans = run_driver(driver, tmp_path, [[0, 256, 1, 1024, SMALL_BUDGET, 0, 40] + local + local, [0, 1, 5, 1024, SMALL_BUDGET, 0, 40] + local + local])
    sizes = []
    for nq, Wt in ((256, 1), (1, 5)):
        ans.take(41)
        why = set()
        want = groups_before(local, nq, Wt, 1024, SMALL_BUDGET, why)
        got = []
        for _ in range(ans.take()):
            got.append(len(ans.take(ans.take())))
            ans.take(5)
        ans.take(len(got) + 1)
        assert got == [len(g["index"]) for g in want]
        sizes.append((got, why))
    assert sizes[0] == ([16, 16, 8], {"survivors"})
    assert sizes[1] == ([12, 12, 12, 4], {"verdicts"})


# ---- the tail-split cut ----

@pytest.mark.parametrize("n_shards", [8, 9, 128])
@pytest.mark.parametrize("pct", [1, 50, 95])
def test_tail_split_cut(driver, tmp_path, n_shards, pct):
    ans = run_driver(driver, tmp_path, [[1, n_shards, pct, K_MAX_GROUP_ARENAS]])
    n0 = ans.take()
    assert 1 <= n0 <= n_shards - 1
    assert n0 == n0_before(n_shards, pct)


def test_tail_split_leaves_short_long_and_unasked_runs_whole(driver, tmp_path):
    runs = [(n, pct) for n in (1, 2, 7, 8, 128, 129, 4096) for pct in (0, 1, 50, 95, 100)]
    ans = run_driver(driver, tmp_path, [[1, n, pct, K_MAX_GROUP_ARENAS] for n, pct in runs])
    for n, pct in runs:
        n0 = ans.take()
        assert n0 == n0_before(n, pct), (n, pct)
        assert (n0 == 0) == (pct == 0 or n < 8 or n > K_MAX_GROUP_ARENAS), (n, pct)
        assert n0 == 0 or 1 <= n0 <= n - 1, (n, pct)


# ---- survivor rows ----

def test_rows_layout_is_what_rows_layout_gave(driver, tmp_path):
    cases = []
    for name, glob in arena_lists().items():
        for nd in (1, 2, 3, 8):
            for nq in N_QUERIES:
                cases.append((f"{name}-nd{nd}-q{nq}", nq, [[shard_blocks(nb, di, nd) for nb in glob] for di in range(nd)]))
    ans = run_driver(driver, tmp_path, [[2, len(local), len(local[0]), nq] + [x for l in local for x in l] for _, nq, local in cases])
    for name, nq, local in cases:
        row_base, arena_off = rows_layout_before(local, nq)
        assert [int(x) for x in ans.take(len(local) + 1)] == row_base, name
        for d in range(len(local)):
            assert [int(x) for x in ans.take(len(local[0]))] == arena_off[d], name
    assert ans.at == len(ans.w)


# ---- the host merge ----

ND = [1, 2, 3, 7, 8, 64, 65]
N_LOCAL = [1, 63, 64, 65, 1000]
Q = 3


def random_part(rng, n_queries, n_local, density):
    """[n_queries][ceil(n_local / 64)] words, bits past n_local zero (as the kernels leave them)"""
    G = (n_local + 63) // 64
    bits = np.zeros((n_queries, G * 64), dtype=np.uint8)
    bits[:, :n_local] = rng.random((n_queries, n_local)) < density
    return bits, np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n_queries, G)


def pack(bits):
    return np.packbits(bits, axis=1, bitorder="little").view("<u8")


def interleave_cases():
    """(name, n_local, di, nd, Gglobal, part words, dst words before, dst words wanted)"""
    rng = np.random.default_rng(4242)
    out = []
    for nd in ND:
        for di in range(nd):
            for n_local in N_LOCAL:
                for density in (0.02, 0.7):
                    n_global = (n_local - 1) * nd + di + 1 + int(rng.integers(0, nd))      # any count that leaves device di n_local blocks
                    assert shard_blocks(n_global, di, nd) == n_local
                    Gg = (n_global + 63) // 64
                    bits, part = random_part(rng, Q, n_local, density)
                    before = (rng.random((Q, Gg * 64)) < 0.3).astype(np.uint8)             # what other devices have merged already
                    before[:, di::nd] = 0
                    want = before.copy()
                    want[:, di: di + n_local * nd: nd] |= bits[:, :n_local]                # THE definition: local bit l is global bit l * nd + di
                    out.append((f"nd{nd}-di{di}-n{n_local}-p{density}", n_local, di, nd, Gg, part, pack(before), pack(want)))
    return out


def check_interleave(driver, tmp_path, body, keep):
    cases = [c for c in interleave_cases() if keep(c[3])]
    ans = run_driver(driver, tmp_path, [np.concatenate([np.asarray([3, body, Q, n_local, di, nd, Gg], dtype="<u8"), part.ravel(), before.ravel()])
                                        for _, n_local, di, nd, Gg, part, before, _ in cases])
    for name, _, _, _, Gg, _, before, want in cases:
        got = ans.take(Q * Gg).reshape(Q, Gg)
        assert np.array_equal(got, want), name
    assert ans.at == len(ans.w)
    return len(cases)


def test_interleave_loop_is_the_definition(driver, tmp_path):
    assert check_interleave(driver, tmp_path, 0, lambda nd: True) == sum(ND) * len(N_LOCAL) * 2


def test_interleave_pdep_is_the_definition(driver, tmp_path):
    if not has_bmi2(driver):
        pytest.skip("this CPU has no BMI2: interleave_shard_pdep cannot run here (interleave_shard takes the loop)")
    # (65 devices take the loop by rule: a deposit mask covers positions below 64)
    assert check_interleave(driver, tmp_path, 1, lambda nd: nd <= 64) == (sum(ND) - 65) * len(N_LOCAL) * 2


def test_interleave_dispatch_is_the_definition(driver, tmp_path):
    check_interleave(driver, tmp_path, 2, lambda nd: True)


def test_merging_a_device_part_is_one_interleave_per_non_empty_shard(driver, tmp_path):
    rng = np.random.default_rng(77)
    cases = []
    for name, glob in arena_lists().items():
        glob = glob[:60]
        for nd in (2, 3, 8):
            for di in range(nd):
                local = [shard_blocks(nb, di, nd) for nb in glob]
                assert 0 in local
                parts, want_rows = [], []
                for nb, nl in zip(glob, local):
                    Gg = (nb + 63) // 64
                    want = np.zeros((Q, Gg * 64), dtype=np.uint8)
                    if nl:
                        bits, part = random_part(rng, Q, nl, 0.4)
                        parts.append(part.ravel())
                        want[:, di: di + nl * nd: nd] = bits[:, :nl]
                    want_rows.append(pack(want).ravel() if Gg else np.zeros(0, dtype="<u8"))
                cases.append((f"{name}-nd{nd}-di{di}", np.concatenate([np.asarray([4, Q, di, nd, len(glob)] + local + glob, dtype="<u8")] + parts),
                              np.concatenate(want_rows)))
    ans = run_driver(driver, tmp_path, [c[1] for c in cases])
    for name, _, want in cases:
        merged, per_shard = ans.take(len(want)), ans.take(len(want))
        assert np.array_equal(merged, per_shard), name
        assert np.array_equal(merged, want), name                   # arena i at out_off[i], query rows of ceil(global / 64) words
    assert ans.at == len(ans.w)
