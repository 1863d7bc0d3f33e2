"""The policy of the resident file-arena cache on the CPU (no GPU): tests/arena_cache_check.cpp drives
bloomsearch_amd/csrc/host/arena_cache.hpp — the class csrc/cache_api.inc adapts to the C ABI, mutex included — built with plain g++.

Script mode, under AddressSanitizer and UBSan: named scenarios with the smallest shapes that reach each rule, then seeded random
sequences of a few thousand operations over 4 keys.  Reference: `Model` below, a restatement of the policy as the header comment of
cache_api.inc writes it down, in dicts and lists.  Every operation's result (lease, arena id, arena blocks, the rows on a hit, the
resident flag, the status, what `have` copied out, the arena ids to free) and the full stats after it are compared line by line; on a
miss the rows are unspecified and not printed.  The program checks by itself, after every operation, that an arena id is handed out
for freeing at most once, never while a lease on it is open, that resident_bytes is the sum over the table, and at the end of every
sequence (all leases released, every key forgotten) that every published id was handed out exactly once.

Thread mode, under ThreadSanitizer: 8 threads, a fixed count of random operations each, a table of atomic flags standing in for the
arenas: freeing finds an arena alive exactly once, a thread holding a lease finds its arena alive until it has released it."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "arena_cache_check.cpp")
COUNTERS = ("hits", "misses", "published", "widenings", "evictions", "forgotten", "rejected_dirty", "rejected_over_budget", "rejected_narrower")
OK, ALREADY_OWNED, UNKNOWN_LEASE, NO_ROOM = 0, 1, 2, 3


def build(dirname, sanitizers):
    exe = os.path.join(str(dirname), "arena_cache_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *sanitizers, "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "bloomsearch_amd", "csrc"), "-o", exe, SRC], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("arena_cache_asan"), ["-fsanitize=address,undefined"])


class Model:
    """The policy, restated.  An entry is a dict; `resident` maps a file key to its entry, `leases` a lease to its entry."""

    def __init__(self):
        self.resident, self.leases, self.owned = {}, {}, set()
        self.budget, self.tick, self.next_lease = 32 << 30, 0, 1
        self.count = dict.fromkeys(COUNTERS, 0)
        self.ever = dict.fromkeys(COUNTERS, 0)          # the counters without the resets: which rules a sequence reached

    def bump(self, counter):
        self.count[counter] += 1
        self.ever[counter] += 1

    def resident_bytes(self):
        return sum(e["bytes"] for e in self.resident.values())

    def take_out(self, e, free):
        """out of the table; freed now when nobody leases it, else by its last release"""
        del self.resident[e["key"]]
        e["dead"] = True
        if e["users"] == 0:
            free.append(e["id"])

    def evict(self, keep, free):
        while self.resident_bytes() > self.budget:
            idle = [e for e in self.resident.values() if e["users"] == 0 and e is not keep]
            if not idle:
                return
            self.take_out(min(idle, key=lambda e: e["last_use"]), free)
            self.bump("evictions")

    def lease(self, e):
        lease, self.next_lease = self.next_lease, self.next_lease + 1
        self.leases[lease] = e
        return lease

    def acquire(self, key, keys):
        e = self.resident.get(key)
        if e is None or any(k not in e["keys"] for k in keys):
            self.bump("misses")
            return {}
        e["users"] += 1
        self.tick += 1
        e["last_use"] = self.tick
        self.bump("hits")
        return {"lease": self.lease(e), "arena": e["id"], "blocks": len(e["keys"]), "rows": [e["keys"].index(k) for k in keys]}

    def have(self, key, cap):
        e = self.resident.get(key)
        if e is None:
            return {"have": "0"}
        n = len(e["keys"])
        if cap == 0:
            return {"have": str(n)}
        if cap < n:
            return {"have": str(n), "status": NO_ROOM}
        return {"have": "%d:%s;%s;%s" % (n, ids(e["keys"]), ids(e["begin"]), ids(e["end"])) if n else "0"}

    def publish(self, key, arena, nbytes, keys, begin, end, clean):
        if arena in self.owned:
            return {"status": ALREADY_OWNED}
        self.owned.add(arena)
        e = {"key": key, "id": arena, "keys": list(keys), "begin": list(begin), "end": list(end), "bytes": nbytes, "users": 1, "last_use": 0, "dead": True}
        out = {"lease": self.lease(e), "free": []}
        old = self.resident.get(key)
        if not clean:
            self.bump("rejected_dirty")
        elif nbytes > self.budget:
            self.bump("rejected_over_budget")
        elif old is not None and len(old["keys"]) > len(keys):
            self.bump("rejected_narrower")
        else:
            if old is not None:
                self.bump("widenings")
                self.take_out(old, out["free"])
            self.tick += 1
            e["last_use"], e["dead"] = self.tick, False
            self.resident[key] = e
            self.evict(e, out["free"])
            self.bump("published")
            out["resident"] = 1
        return out

    def release(self, lease):
        e = self.leases.pop(lease, None)
        if e is None:
            return {"status": UNKNOWN_LEASE}
        free = []
        e["users"] -= 1
        if e["users"] == 0:
            if e["dead"]:
                free.append(e["id"])
            else:
                self.evict(None, free)
        return {"free": free}

    def forget(self, key):
        free = []
        if key in self.resident:
            self.take_out(self.resident[key], free)
            self.bump("forgotten")
        return {"free": free}

    def set_budget(self, nbytes):
        free = []
        self.budget = nbytes
        self.evict(None, free)
        return {"free": free}

    def disown(self, free):
        self.owned -= set(free)

    def stats(self, reset=False):
        dead = {id(e): e["bytes"] for e in self.leases.values() if e["dead"]}
        s = [self.budget, self.resident_bytes(), len(self.resident), len(self.leases), sum(dead.values())] + [self.count[c] for c in COUNTERS]
        if reset:
            self.count = dict.fromkeys(COUNTERS, 0)
        return s


def ids(v):
    return ",".join(str(x) for x in v) if len(v) else "-"


class Script:
    """One sequence: the operations as the program reads them, and the lines the model expects back."""

    def __init__(self, name):
        self.name, self.m = name, Model()
        self.ops, self.want = ["begin " + name], ["begin " + name]
        self.handed = []                 # every lease handed out, in order (release names them by index)
        self.keys = set()

    def step(self, op, r):
        free = sorted(r.get("free", []))
        self.m.disown(free)
        if r.get("lease"):
            self.handed.append(r["lease"])
        self.ops.append(op)
        self.want.append("lease=%d arena=%d blocks=%d rows=%s resident=%d status=%d have=%s got=%s free=%s stats=%s"
                         % (r.get("lease", 0), r.get("arena", 0), r.get("blocks", 0), ids(r["rows"]) if r.get("lease") and "rows" in r else "-",
                            r.get("resident", 0), r.get("status", OK), r.get("have", "-"), r.get("got", "-"), ids(free), ids(self.m.stats())))
        r["free"] = free
        return r

    def acquire(self, key, keys):
        return self.step("acquire %s %d %s" % (key, len(keys), " ".join(map(str, keys))), self.m.acquire(key, keys))

    def have(self, key, cap):
        return self.step("have %s %d" % (key, cap), self.m.have(key, cap))

    def publish(self, key, arena, keys, nbytes=100, clean=True):
        self.keys.add(key)
        begin, end = [10 * k for k in keys], [10 * k + 5 for k in keys]
        op = "publish %s %d %d %d %d %s" % (key, arena, nbytes, int(clean), len(keys), " ".join(map(str, list(keys) + begin + end)))
        return self.step(op, self.m.publish(key, arena, nbytes, keys, begin, end, clean))

    def release(self, index):
        lease = self.handed[index] if index < len(self.handed) else (1 << 40) + index
        return self.step("release %d" % index, self.m.release(lease))

    def forget(self, key):
        return self.step("forget " + key, self.m.forget(key))

    def budget(self, nbytes):
        return self.step("budget %d" % nbytes, self.m.set_budget(nbytes))

    def stats(self, reset):
        return self.step("stats %d" % int(reset), {"got": ids(self.m.stats(reset))})

    def gauge(self, name):
        return self.m.stats()[("budget_bytes", "resident_bytes", "resident_files", "leases", "leased_dead_bytes").index(name)]

    def close(self):
        """every open lease released, every key forgotten: the program then wants every published arena handed out exactly once"""
        for lease in sorted(self.m.leases):
            self.release(self.handed.index(lease))
        for key in sorted(self.keys):
            self.forget(key)
        assert not self.m.owned and not self.m.resident, self.name
        self.ops.append("end")
        self.want.append("end " + self.name)
        return self


def check(exe, tmp_path, scripts):
    path = tmp_path / "script.txt"
    ops = [op for s in scripts for op in s.ops]
    want = [w for s in scripts for w in s.want]
    path.write_text("\n".join(ops) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-6000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) - 1 == len(want) == len(ops)        # no operation is skipped by the comparison
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "operation %d (%s)\n  got  %s\n  want %s" % (i, ops[i], g, w)


# ---- the scenarios: 1 to 4 files, at most 8 blocks each, budgets of two or three entries of 100 bytes ----

def widening_over_an_entry_nobody_leases(s):
    s.publish("f1", 1, [1, 2])
    s.release(0)
    r = s.publish("f1", 2, [1, 2, 3])                    # the dropped entry's last owner is the table itself
    assert r["free"] == [1] and r["resident"] == 1 and s.m.count["widenings"] == 1 and s.gauge("resident_bytes") == 100
    assert s.acquire("f1", [3])["arena"] == 2


def widening_over_an_entry_somebody_leases(s):
    s.publish("f1", 1, [1, 2])
    s.acquire("f1", [2])
    s.release(0)
    r = s.publish("f1", 2, [1, 2, 3, 4])
    assert r["free"] == [] and s.gauge("leased_dead_bytes") == 100 and s.gauge("resident_bytes") == 100       # dead, not freed at the publish
    assert s.release(1)["free"] == [1]                                                                         # ... but by its last release
    assert s.gauge("leased_dead_bytes") == 0


def equal_width_replaces_and_narrower_is_rejected(s):
    s.publish("f1", 1, [1, 2])
    s.release(0)
    r = s.publish("f1", 2, [3, 4])
    assert r["resident"] == 1 and r["free"] == [1] and s.m.count["widenings"] == 1
    r = s.publish("f1", 3, [3])
    assert r.get("resident", 0) == 0 and r["free"] == [] and s.m.count["rejected_narrower"] == 1
    assert s.acquire("f1", [4])["arena"] == 2 and s.acquire("f1", [1]).get("lease", 0) == 0
    assert s.release(2)["free"] == [3]                   # it served its lease only


def dirty_and_over_budget_publishes_serve_their_lease_only(s):
    s.budget(250)
    r = s.publish("f1", 1, [1, 2], clean=False)
    assert r.get("resident", 0) == 0 and s.gauge("resident_files") == 0 and s.gauge("leased_dead_bytes") == 100
    assert s.acquire("f1", [1]).get("lease", 0) == 0
    assert s.release(0)["free"] == [1]
    r = s.publish("f2", 2, [1], nbytes=300)
    assert r.get("resident", 0) == 0 and s.m.count["rejected_over_budget"] == 1
    assert s.release(1)["free"] == [2]
    assert s.publish("f2", 3, [1], nbytes=250)["resident"] == 1          # exactly the budget fits


def an_arena_the_cache_owns_is_refused(s):
    s.publish("f1", 1, [1, 2])
    before = s.m.stats()
    r = s.publish("f2", 1, [1, 2, 3])
    assert r["status"] == ALREADY_OWNED and s.m.stats() == before and len(s.handed) == 1      # no lease, no entry, no counter
    s.have("f2", 0)
    s.release(0)
    assert s.publish("f1", 1, [1, 2, 3])["status"] == ALREADY_OWNED      # resident without a lease: still the cache's
    assert s.forget("f1")["free"] == [1]


def lru_order_over_three_idle_entries(s):
    s.budget(300)
    for i, key in enumerate(("a", "b", "c")):
        s.publish(key, i + 1, [1])
        s.release(i)
    s.acquire("a", [1])                                  # a is now the most recently used
    s.release(3)
    assert s.publish("d", 4, [1])["free"] == [2]
    s.release(4)
    assert s.publish("e", 5, [1])["free"] == [3]
    s.release(5)
    assert s.publish("f", 6, [1])["free"] == [1]


def leased_entries_and_the_one_just_published_are_skipped(s):
    s.budget(200)
    s.publish("a", 1, [1])                               # lease 0 stays open
    s.publish("b", 2, [1])
    s.release(1)
    r = s.publish("c", 3, [1])
    assert r["free"] == [2] and r["resident"] == 1       # a is older but leased
    assert s.budget(100)["free"] == [] and s.gauge("resident_bytes") == 200      # a and c are both in use: the budget is exceeded
    s.release(0)
    assert s.gauge("resident_files") == 1 and s.acquire("c", [1])["arena"] == 3


def the_last_release_runs_the_eviction_the_budget_waited_for(s):
    s.budget(200)
    for i, key in enumerate(("a", "b", "c")):
        assert s.publish(key, i + 1, [1])["free"] == []
    assert s.gauge("resident_bytes") == 300 and s.m.count["evictions"] == 0
    assert s.release(1)["free"] == [2] and s.m.count["evictions"] == 1
    assert s.release(0)["free"] == [] and s.gauge("resident_bytes") == 200


def forget_with_and_without_users(s):
    s.publish("a", 1, [1, 2])
    assert s.forget("a")["free"] == [] and s.gauge("leased_dead_bytes") == 100 and s.gauge("resident_files") == 0
    assert s.acquire("a", [1]).get("lease", 0) == 0
    assert s.release(0)["free"] == [1]
    s.publish("b", 2, [1])
    s.release(1)
    assert s.forget("b")["free"] == [2] and s.m.count["forgotten"] == 2


def forget_of_an_unknown_key(s):
    s.publish("a", 1, [1])
    assert s.forget("nobody")["free"] == [] and s.m.count["forgotten"] == 0 and s.gauge("resident_files") == 1


def double_release_and_release_of_an_unknown_lease(s):
    s.publish("a", 1, [1])
    s.acquire("a", [1])
    assert s.release(0).get("status", OK) == OK
    assert s.release(0)["status"] == UNKNOWN_LEASE
    assert s.release(7)["status"] == UNKNOWN_LEASE       # never handed out
    assert s.gauge("leases") == 1


def set_budget_shrinking_past_several_entries_and_to_zero(s):
    for i, key in enumerate(("a", "b", "c", "d")):
        s.publish(key, i + 1, [1, 2])
        s.release(i)
    s.acquire("b", [2])
    s.release(4)
    assert s.budget(150)["free"] == [1, 3, 4] and s.m.count["evictions"] == 3     # b was used last
    assert s.budget(0)["free"] == [2]
    assert s.publish("a", 5, [1]).get("resident", 0) == 0 and s.m.count["rejected_over_budget"] == 1


def stats_with_reset_keeps_the_five_gauges(s):
    s.budget(1000)
    s.publish("a", 1, [1, 2])
    s.publish("b", 2, [1], clean=False)
    s.acquire("a", [1])
    s.acquire("a", [7])
    s.forget("zzz")
    before = s.m.stats()
    s.stats(True)
    after = s.m.stats()
    assert all(before[:5]) and after[:5] == before[:5] and any(before[5:]) and not any(after[5:])
    s.stats(False)
    s.acquire("a", [2])
    assert s.m.stats()[5] == 1


def have_as_a_size_query_with_too_little_room_and_with_extents(s):
    s.have("a", 0)
    s.have("a", 4)
    s.publish("a", 1, [3, 5, 8])
    assert s.have("a", 0)["have"] == "3"
    assert s.have("a", 2)["status"] == NO_ROOM
    assert s.have("a", 3)["have"] == "3:3,5,8;30,50,80;35,55,85"
    s.have("a", 8)
    s.have("b", 8)


SCENARIOS = [widening_over_an_entry_nobody_leases,          # (first: the path that read freed memory)
             widening_over_an_entry_somebody_leases, equal_width_replaces_and_narrower_is_rejected,
             dirty_and_over_budget_publishes_serve_their_lease_only, an_arena_the_cache_owns_is_refused, lru_order_over_three_idle_entries,
             leased_entries_and_the_one_just_published_are_skipped, the_last_release_runs_the_eviction_the_budget_waited_for,
             forget_with_and_without_users, forget_of_an_unknown_key, double_release_and_release_of_an_unknown_lease,
             set_budget_shrinking_past_several_entries_and_to_zero, stats_with_reset_keeps_the_five_gauges,
             have_as_a_size_query_with_too_little_room_and_with_extents]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
def test_scenario(asan_exe, tmp_path, scenario):
    s = Script(scenario.__name__)
    scenario(s)
    check(asan_exe, tmp_path, [s.close()])


def random_sequence(seed, n_ops):
    rng = random.Random(seed)
    s = Script("random_%d" % seed)
    next_arena = 1
    while len(s.ops) <= n_ops:
        key = "k%d" % rng.randrange(4)
        blocks = sorted(rng.sample(range(1, 9), rng.randrange(0, 5)))
        what = rng.random()
        if what < 0.30:
            if rng.random() < 0.5 and key in s.m.resident:                    # candidates the resident arena covers
                blocks = [k for k in s.m.resident[key]["keys"] if rng.random() < 0.5]
            s.acquire(key, blocks)
        elif what < 0.55 and len(s.m.leases) < 6:
            if rng.random() < 0.5 and key in s.m.resident:                    # a widening load: the union with what is resident
                blocks = sorted(set(blocks) | set(s.m.resident[key]["keys"]))
            arena = next_arena
            if s.m.owned and rng.random() < 0.06:
                arena = rng.choice(sorted(s.m.owned))                         # the cache's already: refused
            else:
                next_arena += 1
            s.publish(key, arena, blocks, nbytes=100 * rng.randrange(1, 5), clean=rng.random() < 0.88)
        elif what < 0.82:
            if rng.random() < 0.06 or not s.handed:
                s.release(rng.randrange(len(s.handed) + 3))                   # any lease ever handed out, or none the cache issued
            elif s.m.leases:
                s.release(s.handed.index(rng.choice(sorted(s.m.leases))))
        elif what < 0.87:
            s.forget(key)
        elif what < 0.92:
            s.budget(rng.choice([0, 250, 600, 1000, 1 << 40]))
        elif what < 0.95:
            s.stats(rng.random() < 0.5)
        else:
            s.have(key, rng.choice([0, 2, 8]))
    return s.close()


def test_random_sequences_against_the_restatement(asan_exe, tmp_path):
    scripts = [random_sequence(seed, 3000) for seed in (1, 2, 3)]
    for s in scripts:
        c = s.m.ever         # every rule was reached
        assert len(s.ops) > 3000 and all(c[k] > 0 for k in COUNTERS), c
    check(asan_exe, tmp_path, scripts)


def test_eight_threads_under_thread_sanitizer(tmp_path):
    exe = build(tmp_path, ["-fsanitize=thread", "-pthread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1")
    for seed in (1, 2):
        r = subprocess.run([exe, "threads", "8", "6000", str(seed)], capture_output=True, text=True, timeout=300, env=env)
        assert "ThreadSanitizer" not in r.stderr and r.returncode == 0, r.stdout + r.stderr[-4000:]
        f = dict(zip(r.stdout.split()[::2], (int(x) for x in r.stdout.split()[1::2])))
        assert f["arenas"] == f["freed"] > 0 and f["hits"] > 0 and f["refused"] > 0 and f["evictions"] > 0, f
