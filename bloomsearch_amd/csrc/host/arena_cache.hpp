// arena_cache.hpp — the policy of the resident file-arena cache, free of any device type: which file arenas stay resident, who holds
// a lease, what is evicted and who frees what.  It knows arena ids and byte counts only; csrc/cache_api.inc is its C-ABI adapter
// (argument checks, the arena's device bytes, the freeing itself), and tests/arena_cache_check.cpp runs the same class on the CPU
// under AddressSanitizer / UBSan and, from 8 threads, under ThreadSanitizer (tests/test_arena_cache_policy.py).
//
// Policy (the entry points are described in cache_api.inc and include/bloomgpu.h):
//   * one resident arena per file key; a publish becomes resident only when it decoded clean, fits the budget by itself and is not
//     narrower (fewer blocks) than what is resident; otherwise it is DEAD from the start: it serves its own lease and goes with it
//   * a resident publish over an entry (widening, or equal width) drops the old entry
//   * above the budget the idle entries (no lease) go, least recently used first; the entry just published never goes; entries in
//     use stay, the budget is exceeded until the release that ends the last lease runs the eviction
//   * a dropped entry is dead: out of the table, its bytes no longer counted; its arena is freed at once when nobody leases it,
//     else by its last release
//   * `owned` holds every arena id the cache will free itself, from its publish until disown() just before the caller frees it
// No operation frees anything: each fills `to_free` with the arena ids the caller must disown() and free, outside the mutex.
// Every id published is handed out this way exactly once, and never while a lease on it is open.
//
// OWNERSHIP RULE: an entry is dropped through a shared_ptr taken BY VALUE (or a copy the caller holds for the duration).  No function
// keeps a reference into a table across an erase of that table: the table's own shared_ptr may be the entry's last owner.
#pragma once
#include "../../../include/bloomgpu.h"   // bsg_arena_cache_stats (plain C)
#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace bsh_cache {

struct FileArena {
    std::string key;
    uint64_t arena_id = 0;
    std::vector<uint64_t> block_keys;             // ascending; row i of the arena is block_keys[i]
    std::vector<uint64_t> sec_begin, sec_end;     // the blocks' section extents in the file (what a widening load re-reads)
    uint64_t bytes = 0;                           // device bytes of the arena (words + descriptors, all shards)
    uint32_t users = 0;
    uint64_t last_use = 0;
    bool dead = false;                            // not (or no longer) in the table: freed by its last release
};

enum Status { kOk = 0, kAlreadyOwned, kUnknownLease, kNoRoom };

class ArenaCache {
public:
    struct Hit { uint64_t lease = 0, arena_id = 0; uint32_t arena_blocks = 0; };       // lease 0: not covered
    struct Published { Status status = kOk; uint64_t lease = 0; bool resident = false; };

    // covered: a lease on the resident arena and out_rows[i] = candidate i's row in it; not covered: a miss is counted (out_rows is
    // then partly written)
    Hit acquire(const std::string &key, const uint64_t *block_keys, uint32_t n_blocks, uint32_t *out_rows)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = resident_.find(key);
        if (it != resident_.end()) {
            const auto &fa = it->second;
            bool covered = true;
            for (uint32_t i = 0; i < n_blocks && covered; ++i) {
                auto p = std::lower_bound(fa->block_keys.begin(), fa->block_keys.end(), block_keys[i]);
                if (p == fa->block_keys.end() || *p != block_keys[i]) covered = false;
                else out_rows[i] = (uint32_t)(p - fa->block_keys.begin());
            }
            if (covered) {
                ++fa->users;
                fa->last_use = ++tick_;
                Hit h{next_lease_++, fa->arena_id, (uint32_t)fa->block_keys.size()};
                leases_.emplace(h.lease, fa);
                ++st_.hits;
                return h;
            }
        }
        ++st_.misses;
        return Hit{};
    }

    // *out_n = blocks of the key's resident arena (0: none).  cap == 0 asks for that only; else the block keys and section extents
    // are copied out, kNoRoom when they do not fit (or an array is missing)
    Status have(const std::string &key, uint64_t *out_block_keys, uint64_t *out_sec_begin, uint64_t *out_sec_end, uint32_t cap, uint32_t *out_n)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = resident_.find(key);
        if (it == resident_.end()) { *out_n = 0; return kOk; }
        const auto &fa = it->second;
        *out_n = (uint32_t)fa->block_keys.size();
        if (cap == 0) return kOk;
        if (cap < *out_n || !out_block_keys || !out_sec_begin || !out_sec_end) return kNoRoom;
        std::copy(fa->block_keys.begin(), fa->block_keys.end(), out_block_keys);
        std::copy(fa->sec_begin.begin(), fa->sec_begin.end(), out_sec_begin);
        std::copy(fa->sec_end.begin(), fa->sec_end.end(), out_sec_end);
        return kOk;
    }

    // the cache owns arena_id from here on (kAlreadyOwned: it did before; nothing is changed) and the caller holds a lease on it
    Published publish(const std::string &key, uint64_t arena_id, uint64_t bytes, const uint64_t *block_keys, const uint64_t *sec_begin,
                      const uint64_t *sec_end, uint32_t n_blocks, bool clean, std::vector<uint64_t> &to_free)
    {
        auto fa = std::make_shared<FileArena>();
        fa->key = key;
        fa->arena_id = arena_id;
        fa->block_keys.assign(block_keys, block_keys + n_blocks);
        fa->sec_begin.assign(sec_begin, sec_begin + n_blocks);
        fa->sec_end.assign(sec_end, sec_end + n_blocks);
        fa->bytes = bytes;
        fa->users = 1;
        std::lock_guard<std::mutex> lk(mu_);
        Published out;
        if (!owned_.insert(arena_id).second) { out.status = kAlreadyOwned; return out; }
        out.lease = next_lease_++;
        leases_.emplace(out.lease, fa);
        auto it = resident_.find(key);
        if (!clean) { fa->dead = true; ++st_.rejected_dirty; }
        else if (fa->bytes > budget_) { fa->dead = true; ++st_.rejected_over_budget; }
        else if (it != resident_.end() && it->second->block_keys.size() > fa->block_keys.size()) { fa->dead = true; ++st_.rejected_narrower; }
        else {
            if (it != resident_.end()) {
                ++st_.widenings;
                if (const uint64_t id = drop(it->second)) to_free.push_back(id);
            }
            fa->last_use = ++tick_;
            resident_[key] = fa;
            bytes_ += fa->bytes;
            evict(fa.get(), to_free);
            out.resident = true;
            ++st_.published;
        }
        return out;
    }

    // ends a lease; the last lease of a dead entry frees its arena, the last lease of a live one runs the eviction the budget waited for
    Status release(uint64_t lease, std::vector<uint64_t> &to_free)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = leases_.find(lease);
        if (it == leases_.end()) return kUnknownLease;
        auto fa = it->second;
        leases_.erase(it);
        if (--fa->users == 0) {
            if (fa->dead) to_free.push_back(fa->arena_id);
            else if (bytes_ > budget_) evict(nullptr, to_free);
        }
        return kOk;
    }

    // the file is gone: out of the table now, freed by its last user
    void forget(const std::string &key, std::vector<uint64_t> &to_free)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = resident_.find(key);
        if (it == resident_.end()) return;
        if (const uint64_t id = drop(it->second)) to_free.push_back(id);
        ++st_.forgotten;
    }

    void set_budget(uint64_t bytes, std::vector<uint64_t> &to_free)
    {
        std::lock_guard<std::mutex> lk(mu_);
        budget_ = bytes;
        evict(nullptr, to_free);
    }

    bool owns(uint64_t arena_id)
    {
        std::lock_guard<std::mutex> lk(mu_);
        return owned_.count(arena_id) != 0;
    }

    // the caller is about to free these (they came out of a to_free list): from here on they are not the cache's
    void disown(const std::vector<uint64_t> &ids)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (uint64_t id : ids) owned_.erase(id);
    }

    // reset clears the counters; the five gauges (budget, resident bytes and files, leases, leased dead bytes) are kept
    void stats(bsg_arena_cache_stats *out, bool reset)
    {
        std::lock_guard<std::mutex> lk(mu_);
        st_.budget_bytes = budget_;
        st_.resident_bytes = bytes_;
        st_.resident_files = resident_.size();
        st_.leases = leases_.size();
        uint64_t held = 0;            // bytes of arenas alive only through their leases (dead entries) — the device memory the table no longer counts
        std::unordered_set<const FileArena *> seen;
        for (auto &kv : leases_)
            if (kv.second->dead && seen.insert(kv.second.get()).second) held += kv.second->bytes;
        st_.leased_dead_bytes = held;
        *out = st_;
        if (reset) {
            const bsg_arena_cache_stats keep = st_;
            st_ = bsg_arena_cache_stats{};
            st_.budget_bytes = keep.budget_bytes; st_.resident_bytes = keep.resident_bytes; st_.resident_files = keep.resident_files;
            st_.leases = keep.leases; st_.leased_dead_bytes = keep.leased_dead_bytes;
        }
    }

protected:      // (the CPU check derives from the class to compare bytes_ with the table's own sum)
    std::mutex mu_;
    std::unordered_map<std::string, std::shared_ptr<FileArena>> resident_;
    std::unordered_map<uint64_t, std::shared_ptr<FileArena>> leases_;
    std::unordered_set<uint64_t> owned_;          // arena ids the cache will free itself (resident, or alive through a lease)
    uint64_t budget_ = 32ull << 30;               // (gpu_engine.go's defaultArenaBudget; bsg_set_arena_budget)
    uint64_t bytes_ = 0, tick_ = 0, next_lease_ = 1;
    bsg_arena_cache_stats st_{};

private:
    // (mutex held) out of the table; returns the arena id to free now, or 0 when its last user will.  BY VALUE: see the ownership rule
    uint64_t drop(std::shared_ptr<FileArena> fa)
    {
        auto it = resident_.find(fa->key);
        if (it != resident_.end() && it->second == fa) resident_.erase(it);
        bytes_ -= fa->bytes;
        fa->dead = true;
        return fa->users == 0 ? fa->arena_id : 0;
    }

    // (mutex held) least recently used entries nobody uses go until the cache fits its budget; `keep` never goes.
    // One pass over the table + a sort of the idle entries (a shrinking budget may let thousands go at once).
    void evict(const FileArena *keep, std::vector<uint64_t> &to_free)
    {
        if (bytes_ <= budget_) return;
        std::vector<std::shared_ptr<FileArena>> idle;
        for (auto &kv : resident_)
            if (kv.second.get() != keep && kv.second->users == 0) idle.push_back(kv.second);
        std::sort(idle.begin(), idle.end(), [](const std::shared_ptr<FileArena> &a, const std::shared_ptr<FileArena> &b) { return a->last_use < b->last_use; });
        for (auto &victim : idle) {
            if (bytes_ <= budget_) return;
            if (const uint64_t id = drop(victim)) to_free.push_back(id);
            ++st_.evictions;
        }
    }
};

}  // namespace bsh_cache
