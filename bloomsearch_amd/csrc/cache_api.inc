// cache_api.inc — the resident file-arena cache (SURVEY 8 f2: "region-resident arena cache across queries").
//
// The reference re-reads and re-parses a file's block-filter sections on EVERY query (blockFilterCursor, file_format.go:511-662,
// consulted per block by evaluateBlockFilters, query_exec.go:546-615).  On the device the decoded filters of a file stay resident
// between queries under one policy that decides which, for how long, and who frees them — inside the library, so that every host
// (the Go overlay's gpu_engine.go, host/engine.hpp, a plain C caller) shares one tested implementation.  The policy itself — the
// tables, leases, eviction, the counters and the mutex — is host/arena_cache.hpp, which knows arena ids and byte counts only and is
// run on the CPU under sanitizers (tests/test_arena_cache_policy.py).  This file is its adapter to the C ABI: the argument checks,
// the arena's device bytes, the policy's statuses as error codes and messages, and the freeing of what the policy lets go:
//
//     bsg_file_arena_acquire   file key + the query's candidate blocks (ascending block keys = RowDataOffset):
//                              covered -> a LEASE on the resident arena + each candidate's row in it; not covered -> lease 0
//     bsg_file_arena_have      what the file's resident arena holds (block keys + section extents): a miss loads the UNION of
//                              that and its own candidates, so two queries alternating over different blocks of one file stop
//                              replacing each other's arena (widening)
//     bsg_file_arena_publish   hands a freshly decoded arena (bsg_arena_stream_finish / bsg_arena_load_sections) to the cache and
//                              returns a lease on it.  It becomes the file's resident arena only when every section decoded
//                              CLEAN (a failed CRC may be a transient bad read: the reference re-reads per query and recovers on
//                              the next one; a cached status would replay the failure until the file is merged away), it fits
//                              the byte budget, and it is not narrower than what a concurrent query published meanwhile;
//                              otherwise it serves this lease only and is freed by its release
//     bsg_file_arena_release   ends a lease; the last lease of a dead entry frees its arena
//     bsg_file_arena_forget    the file was tombstoned (merge.go:178-185, TombstoneFile): out of the table now, freed by its last user
//     bsg_set_arena_budget     bytes of device memory the resident arenas may hold; above it the least recently used entries
//                              NOBODY holds a lease on are freed (an entry in use is never evicted: the budget is exceeded until
//                              those queries finish — the release that ends the last lease runs the eviction)
//
// An arena the cache holds is owned by the cache: the caller must not bsg_arena_free it.  Leases are plain ids (double release
// and unknown ids are BSG_E_NOTFOUND).  Everything is guarded by the policy's one mutex; device memory is freed outside it.

struct bsg_arena_cache : bsh_cache::ArenaCache {};

namespace {

uint64_t arena_device_bytes(const Arena &a)
{
    uint64_t b = 0;
    for (auto &s : a.shards) b += s.n_words * 8 + (uint64_t)s.n_blocks * 3 * sizeof(DevDesc);
    return b;
}

bool strictly_ascending(const uint64_t *v, uint32_t n)
{
    for (uint32_t i = 1; i < n; ++i) if (v[i] <= v[i - 1]) return false;
    return true;
}

int32_t arena_free_by_id(bsg_ctx *ctx, uint64_t arena_id);   // bloomgpu.hip

// frees arenas the cache has let go of (outside the cache mutex: freeing waits for the devices)
void cache_free_ids(bsg_ctx *ctx, const std::vector<uint64_t> &ids)
{
    if (ids.empty()) return;
    ctx->cache->disown(ids);
    for (uint64_t id : ids) (void)arena_free_by_id(ctx, id);
}

bool cache_owns(bsg_ctx *ctx, uint64_t arena_id) { return ctx->cache->owns(arena_id); }

std::shared_ptr<bsg_arena_cache> arena_cache_create() { return std::make_shared<bsg_arena_cache>(); }

void arena_cache_destroy(bsg_ctx *ctx)      // bsg_close: the arenas themselves go with the context's handle table
{
    ctx->cache.reset();
}

}  // namespace

extern "C" {

int32_t bsg_set_arena_budget(bsg_ctx *ctx, uint64_t bytes)
{
    BSG_ENTER(ctx);
    std::vector<uint64_t> to_free;
    ctx->cache->set_budget(bytes, to_free);
    cache_free_ids(ctx, to_free);
    return BSG_OK;
}

int32_t bsg_file_arena_acquire(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, const uint64_t *block_keys, uint32_t n_blocks,
                               uint64_t *out_lease, uint64_t *out_arena_id, uint32_t *out_arena_blocks, uint32_t *out_rows)
{
    BSG_ENTER(ctx);
    if ((!key && key_len) || (!block_keys && n_blocks) || !out_lease || !out_arena_id || (!out_rows && n_blocks))
        return fail(BSG_E_INVALID, "bsg_file_arena_acquire: null argument");
    if (!strictly_ascending(block_keys, n_blocks)) return fail(BSG_E_INVALID, "bsg_file_arena_acquire: block keys are not strictly ascending");
    const bsh_cache::ArenaCache::Hit h = ctx->cache->acquire(std::string((const char *)key, key_len), block_keys, n_blocks, out_rows);
    *out_lease = h.lease;
    *out_arena_id = h.arena_id;
    if (out_arena_blocks) *out_arena_blocks = h.arena_blocks;
    return BSG_OK;
}

int32_t bsg_file_arena_have(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, uint64_t *out_block_keys, uint64_t *out_sec_begin,
                            uint64_t *out_sec_end, uint32_t cap, uint32_t *out_n)
{
    BSG_ENTER(ctx);
    if ((!key && key_len) || !out_n) return fail(BSG_E_INVALID, "bsg_file_arena_have: null argument");
    if (ctx->cache->have(std::string((const char *)key, key_len), out_block_keys, out_sec_begin, out_sec_end, cap, out_n) == bsh_cache::kNoRoom)
        return fail(BSG_E_INVALID, "bsg_file_arena_have: room for %u blocks, the resident arena holds %u", cap, *out_n);
    return BSG_OK;
}

int32_t bsg_file_arena_publish(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, uint64_t arena_id, const uint64_t *block_keys,
                               const uint64_t *sec_begin, const uint64_t *sec_end, const int32_t *status, uint32_t n_blocks,
                               uint64_t *out_lease, int32_t *out_resident)
{
    BSG_ENTER(ctx);
    if ((!key && key_len) || (n_blocks && (!block_keys || !sec_begin || !sec_end)) || !out_lease)
        return fail(BSG_E_INVALID, "bsg_file_arena_publish: null argument");
    if (!strictly_ascending(block_keys, n_blocks)) return fail(BSG_E_INVALID, "bsg_file_arena_publish: block keys are not strictly ascending");
    std::shared_ptr<Arena> a;
    if (int32_t rc = get_arena(ctx, arena_id, a)) return rc;
    if (a->n_blocks != n_blocks) return fail(BSG_E_INVALID, "bsg_file_arena_publish: the arena holds %u blocks, %u keys given", a->n_blocks, n_blocks);
    bool clean = true;
    for (uint32_t i = 0; status && i < n_blocks; ++i) clean = clean && status[i] == 0;
    std::vector<uint64_t> to_free;
    const bsh_cache::ArenaCache::Published p = ctx->cache->publish(std::string((const char *)key, key_len), arena_id, arena_device_bytes(*a), block_keys,
                                                                   sec_begin, sec_end, n_blocks, clean, to_free);
    if (p.status == bsh_cache::kAlreadyOwned) return fail(BSG_E_INVALID, "bsg_file_arena_publish: arena %llu is already the cache's", (unsigned long long)arena_id);
    *out_lease = p.lease;
    if (out_resident) *out_resident = p.resident ? 1 : 0;
    cache_free_ids(ctx, to_free);
    return BSG_OK;
}

int32_t bsg_file_arena_release(bsg_ctx *ctx, uint64_t lease)
{
    BSG_ENTER(ctx);
    std::vector<uint64_t> to_free;
    if (ctx->cache->release(lease, to_free) == bsh_cache::kUnknownLease) return fail(BSG_E_NOTFOUND, "unknown file-arena lease %llu", (unsigned long long)lease);
    cache_free_ids(ctx, to_free);
    return BSG_OK;
}

int32_t bsg_file_arena_forget(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len)
{
    BSG_ENTER(ctx);
    if (!key && key_len) return fail(BSG_E_INVALID, "bsg_file_arena_forget: null key");
    std::vector<uint64_t> to_free;
    ctx->cache->forget(std::string((const char *)key, key_len), to_free);
    cache_free_ids(ctx, to_free);
    return BSG_OK;
}

int32_t bsg_arena_cache_stats_read(bsg_ctx *ctx, bsg_arena_cache_stats *out, int32_t reset)
{
    BSG_ENTER(ctx);
    if (!out) return fail(BSG_E_INVALID, "out is null");
    ctx->cache->stats(out, reset != 0);
    return BSG_OK;
}

}  // extern "C"
