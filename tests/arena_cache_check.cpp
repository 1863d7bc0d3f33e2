// Host driver of the resident file-arena cache's policy (bloomsearch_amd/csrc/host/arena_cache.hpp — the class csrc/cache_api.inc
// adapts to the C ABI), built with plain g++ by tests/test_arena_cache_policy.py: under -fsanitize=address,undefined for the script
// mode, under -fsanitize=thread for the thread mode.
//
// Script mode:  arena_cache_check <script>.  One operation per line, run on one cache per sequence:
//     begin NAME | acquire KEY N k.. | have KEY CAP | publish KEY ID BYTES CLEAN N k.. b.. e.. | release I | forget KEY | budget BYTES
//     | stats RESET | end
// release I names the I-th lease this sequence handed out (0-based; one the sequence has not handed out yet stands for a lease the
// cache never issued).  After each operation one line: what it returned (lease or 0, arena id, arena blocks, the rows on a hit,
// resident flag, status, what have copied out, the stats a stats operation read), the arena ids to free sorted, and the full stats.
// Checked here after every operation: an id is handed out for freeing at most once, only after it was published and never while a
// lease on it is open; resident_bytes is the sum over the table.  `end` (after the script has released every lease and forgotten
// every key): every id published was handed out exactly once.  Exit 3 with a message when a condition fails.
//
// Thread mode:  arena_cache_check threads T OPS SEED.  T threads do OPS random operations each on one cache over 4 keys; a table of
// atomic flags, one per arena id, stands in for the arenas: freeing (disown, then the flag) must find it alive exactly once, and a
// thread holding a lease must find its arena alive until it has released it.
#include "host/arena_cache.hpp"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <thread>

using bsh_cache::ArenaCache;

namespace {

[[noreturn]] void die(const std::string &what)
{
    fprintf(stderr, "arena_cache_check: %s\n", what.c_str());
    exit(3);
}

struct Probe : ArenaCache {
    bool bytes_are_the_tables_sum()
    {
        std::lock_guard<std::mutex> lk(mu_);
        uint64_t sum = 0;
        for (auto &kv : resident_) {
            if (kv.second->dead || kv.second->key != kv.first) return false;
            sum += kv.second->bytes;
        }
        return sum == bytes_;
    }
};

std::string list(const std::vector<uint64_t> &v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s.empty() ? "-" : s;
}

std::string stats_text(const bsg_arena_cache_stats &s)
{
    const uint64_t f[14] = {s.budget_bytes, s.resident_bytes, s.resident_files, s.leases, s.leased_dead_bytes, s.hits, s.misses, s.published,
                            s.widenings, s.evictions, s.forgotten, s.rejected_dirty, s.rejected_over_budget, s.rejected_narrower};
    return list(std::vector<uint64_t>(f, f + 14));
}

struct Sequence {                                  // one cache and what this program knows about its arenas
    Probe cache;
    std::string name;
    std::vector<uint64_t> leases;                  // every lease handed out, in order
    std::map<uint64_t, uint64_t> open;             // open lease -> its arena id
    std::map<uint64_t, uint32_t> open_on;          // arena id -> open leases on it
    std::set<uint64_t> published, freed;

    void took_lease(uint64_t lease, uint64_t id)
    {
        leases.push_back(lease);
        open[lease] = id;
        ++open_on[id];
    }
    void handed_out(std::vector<uint64_t> &ids, const std::string &at)
    {
        std::sort(ids.begin(), ids.end());
        for (uint64_t id : ids) {
            if (!published.count(id)) die(at + ": arena " + std::to_string(id) + " was never published");
            if (!freed.insert(id).second) die(at + ": arena " + std::to_string(id) + " handed out for freeing twice");
            if (open_on[id] != 0) die(at + ": arena " + std::to_string(id) + " handed out while a lease on it is open");
            if (!cache.owns(id)) die(at + ": arena " + std::to_string(id) + " handed out but not the cache's");
        }
        cache.disown(ids);
        if (!cache.bytes_are_the_tables_sum()) die(at + ": resident_bytes is not the sum over the table");
    }
};

int run_script(const char *path)
{
    std::ifstream in(path);
    if (!in) return 2;
    std::unique_ptr<Sequence> s;
    std::string line;
    for (uint32_t n = 1; std::getline(in, line); ++n) {
        std::istringstream t(line);
        std::string op, key;
        t >> op;
        const std::string at = "line " + std::to_string(n) + " (" + line.substr(0, 40) + ")";
        if (op == "begin") {
            s.reset(new Sequence);
            t >> s->name;
            printf("begin %s\n", s->name.c_str());
            continue;
        }
        if (!s) die(at + ": no sequence begun");
        if (op == "end") {
            if (!s->open.empty()) die(at + ": the script left leases open");
            if (s->freed != s->published) die(at + ": " + std::to_string(s->published.size()) + " arenas published, " + std::to_string(s->freed.size()) + " handed out for freeing");
            printf("end %s\n", s->name.c_str());
            s.reset();
            continue;
        }
        uint64_t lease = 0, arena = 0, blocks = 0;
        int resident = 0, status = 0;
        std::string rows = "-", have = "-", got = "-";
        std::vector<uint64_t> to_free;
        if (op == "acquire") {
            uint32_t nk = 0;
            t >> key >> nk;
            std::vector<uint64_t> keys(nk);
            for (auto &k : keys) t >> k;
            std::vector<uint32_t> r(nk, 0xFFFFFFFFu);
            const ArenaCache::Hit h = s->cache.acquire(key, keys.data(), nk, r.data());
            lease = h.lease; arena = h.arena_id; blocks = h.arena_blocks;
            if (h.lease) {
                s->took_lease(h.lease, h.arena_id);
                rows = list(std::vector<uint64_t>(r.begin(), r.end()));
            }
        } else if (op == "have") {
            uint32_t cap = 0, nh = 0;
            t >> key >> cap;
            std::vector<uint64_t> k(cap, ~0ull), b(cap, ~0ull), e(cap, ~0ull);
            status = s->cache.have(key, k.data(), b.data(), e.data(), cap, &nh);
            have = std::to_string(nh);
            if (cap && nh && status == bsh_cache::kOk) {
                k.resize(nh); b.resize(nh); e.resize(nh);
                have += ":" + list(k) + ";" + list(b) + ";" + list(e);
            }
        } else if (op == "publish") {
            uint64_t id = 0, bytes = 0;
            int clean = 0;
            uint32_t nk = 0;
            t >> key >> id >> bytes >> clean >> nk;
            std::vector<uint64_t> k(nk), b(nk), e(nk);
            for (auto &x : k) t >> x;
            for (auto &x : b) t >> x;
            for (auto &x : e) t >> x;
            const ArenaCache::Published p = s->cache.publish(key, id, bytes, k.data(), b.data(), e.data(), nk, clean != 0, to_free);
            lease = p.lease; resident = p.resident; status = p.status;
            if (p.status == bsh_cache::kOk) {
                if (!s->published.insert(id).second) die(at + ": arena " + std::to_string(id) + " accepted twice");
                s->took_lease(p.lease, id);
            } else if (p.lease || p.resident || !to_free.empty()) die(at + ": a refused publish returned something");
        } else if (op == "release") {
            uint64_t i = 0;
            t >> i;
            const uint64_t l = i < s->leases.size() ? s->leases[i] : (1ull << 40) + i;
            status = s->cache.release(l, to_free);
            auto it = s->open.find(l);
            if ((status == bsh_cache::kOk) != (it != s->open.end())) die(at + ": release answered " + std::to_string(status));
            if (it != s->open.end()) { --s->open_on[it->second]; s->open.erase(it); }
        } else if (op == "forget") {
            t >> key;
            s->cache.forget(key, to_free);
        } else if (op == "budget") {
            uint64_t bytes = 0;
            t >> bytes;
            s->cache.set_budget(bytes, to_free);
        } else if (op == "stats") {
            int reset = 0;
            t >> reset;
            bsg_arena_cache_stats st;
            s->cache.stats(&st, reset != 0);
            got = stats_text(st);
        } else die(at + ": unknown operation");
        if (t.fail()) die(at + ": short line");
        s->handed_out(to_free, at);
        bsg_arena_cache_stats st;
        s->cache.stats(&st, false);
        printf("lease=%llu arena=%llu blocks=%llu rows=%s resident=%d status=%d have=%s got=%s free=%s stats=%s\n", (unsigned long long)lease,
               (unsigned long long)arena, (unsigned long long)blocks, rows.c_str(), resident, status, have.c_str(), got.c_str(), list(to_free).c_str(),
               stats_text(st).c_str());
    }
    if (s) die("the script ends inside sequence " + s->name);
    return 0;
}

// ---- thread mode ----

struct Shared {
    Probe cache;
    std::unique_ptr<std::atomic<int>[]> alive;      // the stand-in arena table: 1 from its creation until it is freed
    std::atomic<uint64_t> next_id{1}, freed{0}, hits{0}, refused{0};
    uint64_t n_ids = 0;

    void free_ids(const std::vector<uint64_t> &ids)                 // cache_api.inc's cache_free_ids over the stand-in table
    {
        if (ids.empty()) return;
        cache.disown(ids);
        for (uint64_t id : ids) {
            int was = 1;
            if (id == 0 || id >= n_ids || !alive[id].compare_exchange_strong(was, 0)) die("arena " + std::to_string(id) + " freed while not alive");
            freed.fetch_add(1);
        }
    }
};

uint64_t next_random(uint64_t &x)                                   // splitmix64
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void caller(Shared &sh, uint32_t ops, uint64_t seed)
{
    static const uint64_t budgets[5] = {0, 300, 700, 1500, 1ull << 40};
    uint64_t rng = seed;
    std::vector<std::pair<uint64_t, uint64_t>> held;                // (lease, arena id)
    auto release_one = [&](size_t i) {
        if (sh.alive[held[i].second].load() != 1) die("a leased arena is not alive");
        if (!sh.cache.owns(held[i].second)) die("a leased arena is not the cache's");
        std::vector<uint64_t> to_free;
        if (sh.cache.release(held[i].first, to_free) != bsh_cache::kOk) die("an open lease is unknown");
        held.erase(held.begin() + i);
        sh.free_ids(to_free);
    };
    for (uint32_t n = 0; n < ops; ++n) {
        const uint64_t r = next_random(rng);
        const std::string key = "file" + std::to_string((r >> 8) % 4);
        const uint32_t what = r % 16;
        std::vector<uint64_t> to_free;
        if (what < 9 && held.size() < 4) {                          // a query: acquire; on a miss load the union and publish it
            std::vector<uint64_t> want;
            for (uint32_t b = 0; b < 8; ++b) if ((r >> (16 + b)) & 1) want.push_back(100 * (b + 1));
            std::vector<uint32_t> rows(want.size());
            const ArenaCache::Hit h = sh.cache.acquire(key, want.data(), (uint32_t)want.size(), rows.data());
            if (h.lease) {
                if (sh.alive[h.arena_id].load() != 1) die("acquire leased an arena that is not alive");
                held.emplace_back(h.lease, h.arena_id);
                sh.hits.fetch_add(1);
                continue;
            }
            uint64_t k[8], b[8], e[8];
            uint32_t nh = 0;
            if (sh.cache.have(key, k, b, e, 8, &nh) != bsh_cache::kOk) die("have found no room for 8 blocks");
            std::set<uint64_t> all(want.begin(), want.end());
            all.insert(k, k + nh);
            std::vector<uint64_t> keys(all.begin(), all.end()), ext(keys.size(), 0);
            const uint64_t id = sh.next_id.fetch_add(1);
            if (id >= sh.n_ids) die("more arenas than operations");
            sh.alive[id].store(1);
            const ArenaCache::Published p = sh.cache.publish(key, id, 100 * (1 + (r >> 32) % 4), keys.data(), ext.data(), ext.data(), (uint32_t)keys.size(),
                                                             (r >> 40) % 8 != 0, to_free);
            if (p.status != bsh_cache::kOk || !p.lease) die("a fresh arena was refused");
            held.emplace_back(p.lease, id);
        } else if (what < 13) {
            if (held.empty()) continue;
            release_one((r >> 16) % held.size());
        } else if (what == 13) {
            sh.cache.forget(key, to_free);
        } else if (what == 14) {
            sh.cache.set_budget(budgets[(r >> 16) % 5], to_free);
        } else {                                                    // an arena the cache has is refused, and nothing comes of it
            if (held.empty()) continue;
            const uint64_t id = held[(r >> 16) % held.size()].second, k = 100;
            const ArenaCache::Published p = sh.cache.publish(key, id, 100, &k, &k, &k, 1, true, to_free);
            if (p.status != bsh_cache::kAlreadyOwned || p.lease || !to_free.empty()) die("a leased arena was published again");
            sh.refused.fetch_add(1);
        }
        sh.free_ids(to_free);
    }
    while (!held.empty()) release_one(held.size() - 1);
}

int run_threads(uint32_t n_threads, uint32_t ops, uint64_t seed)
{
    Shared sh;
    sh.n_ids = (uint64_t)n_threads * ops + 2;
    sh.alive.reset(new std::atomic<int>[sh.n_ids]);
    for (uint64_t i = 0; i < sh.n_ids; ++i) sh.alive[i].store(0);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n_threads; ++i) th.emplace_back(caller, std::ref(sh), ops, seed * 1000003ull + i);
    for (auto &t : th) t.join();
    std::vector<uint64_t> to_free;
    for (uint32_t f = 0; f < 4; ++f) sh.cache.forget("file" + std::to_string(f), to_free);
    sh.free_ids(to_free);
    const uint64_t made = sh.next_id.load() - 1;
    for (uint64_t id = 1; id <= made; ++id) {
        if (sh.alive[id].load() != 0) die("arena " + std::to_string(id) + " was never freed");
        if (sh.cache.owns(id)) die("arena " + std::to_string(id) + " is still the cache's");
    }
    bsg_arena_cache_stats st;
    sh.cache.stats(&st, false);
    if (!sh.cache.bytes_are_the_tables_sum() || st.resident_bytes || st.resident_files || st.leases || st.leased_dead_bytes) die("the cache does not end empty");
    printf("arenas %llu freed %llu hits %llu refused %llu published %llu evictions %llu\n", (unsigned long long)made, (unsigned long long)sh.freed.load(),
           (unsigned long long)sh.hits.load(), (unsigned long long)sh.refused.load(), (unsigned long long)st.published, (unsigned long long)st.evictions);
    return made == sh.freed.load() ? 0 : 3;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2) return run_script(argv[1]);
    if (argc == 5 && std::string(argv[1]) == "threads")
        return run_threads((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), strtoull(argv[4], nullptr, 10));
    return 2;
}
