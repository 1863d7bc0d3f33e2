// stream_api.inc — blockFilterCursor on the device side (a9: file_format.go:511-662, planBlockFilterReads :535-555).
//
// The reference reads a file's contiguous block-filter region in <= 4 MiB chunks, starting at the consulted block's
// section and skipping gaps wider than the cap, and parses each section when its block is reached.  Here the host hands
// the same chunks over AS IT READS THEM:
//     bsg_arena_stream_begin   the candidate blocks' section extents (file offsets, from the footer metadata)
//     bsg_arena_stream_append  one chunk of the file (any chunking; ranges nobody appends are simply never read)
//     bsg_arena_stream_finish  per-block status + the resident arena
// and everything inside a section — CRC32C, flags, lengths, (m, k), the big-endian words — is parsed and decoded on the
// device (k_decode_sections), section by section as soon as its last byte has landed: the copy of chunk i+1 (staging
// memcpy + DMA on the copy stream) overlaps the decode of chunk i (compute stream).  Contexts on several devices shard
// the blocks round-robin; every device receives the chunks over its own link and decodes only its own sections.
// bsg_arena_load_sections is the same path with the whole region appended in 4 MiB chunks.

namespace {

constexpr uint64_t kStreamChunk = 4ull << 20;      // the reference's read cap (file_format.go:484)
constexpr int32_t kSectionUnread = -7;             // the section's bytes were never (completely) appended

struct StreamDev {
    uint8_t *d_region = nullptr;                   // image of file bytes [base, base + span)
    bsg::SectionSlot *d_slots = nullptr;
    int32_t *d_status = nullptr;
    uint64_t *d_crc_acc = nullptr;                 // k_decode_sections: per slot, the XOR of the slices' checksum contributions + their arrival flags
    uint8_t *staging[2] = {nullptr, nullptr};      // pinned; the caller's bytes are copied out before append returns
    hipEvent_t staged_free[2] = {nullptr, nullptr};
    bool staged_busy[2] = {false, false};
    hipEvent_t copied = nullptr;
    hipStream_t copy = nullptr;
    uint32_t stage_next = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timers;
    ArenaShard shard;
    std::vector<bsg::SectionSlot> slots;           // this device's sections, ascending by begin
    std::vector<uint64_t> ends;                    // begin + len of each (same order)
    std::vector<uint32_t> global_block;            // slot -> caller's block index
    std::vector<uint8_t> decoded;
};

struct ArenaStream {
    uint32_t n_blocks = 0;
    uint64_t base = 0, span = 0;
    std::vector<std::pair<uint64_t, uint64_t>> have;   // received [lo, hi) file ranges, merged, ascending
    std::vector<StreamDev> dev;
    std::shared_ptr<Arena> arena;
};

void free_stream_dev(Device &d, StreamDev &s, bool keep_arena)
{
    (void)hipSetDevice(d.id);
    if (s.copy) (void)hipStreamSynchronize(s.copy);
    (void)hipStreamSynchronize(d.stream);
    if (s.d_region) d.pool.free(s.d_region);
    if (s.d_slots) d.pool.free(s.d_slots);
    if (s.d_status) d.pool.free(s.d_status);
    if (s.d_crc_acc) d.pool.free(s.d_crc_acc);
    for (int i = 0; i < 2; ++i)
        if (s.staging[i]) d.idle_staging.push_back(s.staging[i]);   // pinned allocations cost ~1 ms each: kept for the next stream
    if (s.copy && s.copied && s.staged_free[0] && s.staged_free[1] && d.idle_kits.size() < 64)      // (the copy stream was drained above)
        d.idle_kits.push_back(Device::StreamKit{s.copy, s.copied, {s.staged_free[0], s.staged_free[1]}});
    else {
        for (int i = 0; i < 2; ++i) if (s.staged_free[i]) (void)hipEventDestroy(s.staged_free[i]);
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.copy) (void)hipStreamDestroy(s.copy);
    }
    for (auto &t : s.timers) { (void)hipEventDestroy(t.first); (void)hipEventDestroy(t.second); }
    s.timers.clear();
    if (!keep_arena) {
        if (s.shard.d_words) (void)hipFree(s.shard.d_words);
        if (s.shard.d_desc) (void)hipFree(s.shard.d_desc);
    }
    s = StreamDev{};
}

void free_stream(bsg_ctx *ctx, ArenaStream &st, bool keep_arena)
{
    for (size_t di = 0; di < st.dev.size(); ++di) {
        std::lock_guard<std::mutex> lk(ctx->devs[di]->mu);
        free_stream_dev(*ctx->devs[di], st.dev[di], keep_arena);
    }
}

int32_t get_stream(bsg_ctx *ctx, uint64_t id, std::shared_ptr<ArenaStream> &out)
{
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    auto it = ctx->streams.find(id);
    if (it == ctx->streams.end()) return fail(BSG_E_NOTFOUND, "unknown arena stream id %llu", (unsigned long long)id);
    out = it->second;
    return BSG_OK;
}

void free_all_streams(bsg_ctx *ctx)
{
    for (auto &kv : ctx->streams) free_stream(ctx, *kv.second, false);
    ctx->streams.clear();
}

// decode every section of device di that [lo, hi) (a merged received range) now covers completely
int32_t decode_ready(Device &d, StreamDev &s, uint64_t lo, uint64_t hi, uint64_t chunk_lo, uint64_t chunk_hi, uint64_t base)
{
    // candidates overlap the chunk just appended: first slot whose end > chunk_lo
    const uint64_t clo = chunk_lo - base, chi = chunk_hi - base, rlo = lo - base, rhi = hi - base;
    size_t i = std::upper_bound(s.ends.begin(), s.ends.end(), clo) - s.ends.begin();
    uint32_t run_first = 0, run_len = 0;
    bool waited = false;
    auto flush = [&]() -> int32_t {
        if (!run_len) return BSG_OK;
        if (!waited) { HIP_TRY(hipStreamWaitEvent(d.stream, s.copied, 0)); waited = true; }
        for (uint32_t r0 = run_first; r0 < run_first + run_len; r0 += 65535u) {          // (grid.y holds 65 535 sections)
            const uint32_t n = std::min(65535u, run_first + run_len - r0);
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            s.timers.emplace_back(a, b);
            uint32_t max_splits = 1;              // slices (workgroups) of the run's largest section
            for (uint32_t r = r0; r < r0 + n; ++r) max_splits = std::max(max_splits, bsg::decode_splits(s.slots[r].len));
            hipExtLaunchKernelGGL(bsg::k_decode_sections, dim3(max_splits, n), dim3(bsg::kDecodeLaunchThreads), 0, d.stream, a, b, 0,
                                  (const uint8_t *)s.d_region, (const bsg::SectionSlot *)s.d_slots, r0, (const bsg::CrcConsts *)d.d_crc,
                                  s.shard.d_words, s.shard.d_desc, s.d_status, bsg::DecodeScratch{s.d_crc_acc});
            HIP_TRY(hipGetLastError());
        }
        run_len = 0;
        return BSG_OK;
    };
    for (; i < s.slots.size() && s.slots[i].begin < chi; ++i) {
        const bool ready = !s.decoded[i] && s.slots[i].len != 0 && s.slots[i].begin >= rlo && s.ends[i] <= rhi;
        if (ready) {
            s.decoded[i] = 1;
            if (run_len && run_first + run_len == i) { ++run_len; continue; }
            if (int32_t rc = flush()) return rc;
            run_first = (uint32_t)i; run_len = 1;
        } else if (run_len) {
            if (int32_t rc = flush()) return rc;
        }
    }
    return flush();
}

// borrow: the caller's memory stays valid until the stream is finished (bsg_arena_load_sections): no staging copy
int32_t stream_append(bsg_ctx *ctx, ArenaStream &st, uint64_t file_off, const uint8_t *bytes, uint64_t len, bool borrow = false)
{
    // clip to the extent the stream was opened for
    uint64_t lo = std::max(file_off, st.base), hi = std::min(file_off + len, st.base + st.span);
    if (hi <= lo) return BSG_OK;
    bytes += lo - file_off;
    // only bytes that have not arrived yet are copied: a section's first complete delivery is final (its decode may
    // already be running on the compute stream — a second copy of the same bytes on the copy stream would race it, and a
    // "corrected" re-send could not change the block's status any more)
    std::vector<std::pair<uint64_t, uint64_t>> fresh;
    {
        uint64_t cur = lo;
        for (const auto &h : st.have) {                    // ascending, disjoint
            if (h.second <= cur) continue;
            if (h.first >= hi) break;
            if (h.first > cur) fresh.emplace_back(cur, h.first);
            cur = std::max(cur, h.second);
            if (cur >= hi) break;
        }
        if (cur < hi) fresh.emplace_back(cur, hi);
    }
    if (fresh.empty()) return BSG_OK;
    // merge into the received ranges
    auto it = st.have.begin();
    uint64_t mlo = lo, mhi = hi;
    std::vector<std::pair<uint64_t, uint64_t>> merged;
    for (; it != st.have.end(); ++it) {
        if (it->second < mlo || it->first > mhi) merged.push_back(*it);
        else { mlo = std::min(mlo, it->first); mhi = std::max(mhi, it->second); }
    }
    merged.emplace_back(mlo, mhi);
    std::sort(merged.begin(), merged.end());
    st.have.swap(merged);
    for (size_t di = 0; di < st.dev.size(); ++di) {
        Device &d = *ctx->devs[di];
        StreamDev &s = st.dev[di];
        if (s.slots.empty()) continue;
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) return rc;
        for (const auto &fr : fresh)
            for (uint64_t o = fr.first; o < fr.second; o += kStreamChunk) {
                const uint64_t n = std::min(kStreamChunk, fr.second - o);
                if (borrow) {
                    HIP_TRY(hipMemcpyAsync(s.d_region + (o - st.base), bytes + (o - lo), n, hipMemcpyHostToDevice, s.copy));
                    continue;
                }
                const uint32_t b = s.stage_next++ & 1u;
                if (s.staged_busy[b]) { HIP_TRY(hipEventSynchronize(s.staged_free[b])); s.staged_busy[b] = false; }
                memcpy(s.staging[b], bytes + (o - lo), n);      // the caller's memory is only valid during this call
                HIP_TRY(hipMemcpyAsync(s.d_region + (o - st.base), s.staging[b], n, hipMemcpyHostToDevice, s.copy));
                HIP_TRY(hipEventRecord(s.staged_free[b], s.copy));
                s.staged_busy[b] = true;
            }
        HIP_TRY(hipEventRecord(s.copied, s.copy));
        if (int32_t rc = decode_ready(d, s, mlo, mhi, lo, hi, st.base)) return rc;
    }
    return BSG_OK;
}

int32_t stream_begin(bsg_ctx *ctx, const uint64_t *sec_begin, const uint64_t *sec_end, uint32_t n_blocks, std::shared_ptr<ArenaStream> &out)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    auto st = std::make_shared<ArenaStream>();
    st->n_blocks = n_blocks;
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        if (sec_end[b] < sec_begin[b]) return fail(BSG_E_INVALID, "section %u ends before it begins", b);
        if (sec_end[b] - sec_begin[b] > 0xFFFFFFFFull) return fail(BSG_E_INVALID, "section %u is larger than 4 GiB", b);
        if (sec_end[b] == sec_begin[b]) continue;
        lo = std::min(lo, sec_begin[b]); hi = std::max(hi, sec_end[b]);
    }
    if (hi <= lo) { lo = hi = 0; }
    st->base = lo; st->span = hi - lo;
    st->arena = std::make_shared<Arena>();
    st->arena->n_blocks = n_blocks;
    st->arena->shards.resize(nd);
    st->dev.resize(nd);
    // every device's slot table is laid out (and rejected, if the metadata is bad) before anything is allocated
    for (uint32_t di = 0; di < nd; ++di) {
        StreamDev &s = st->dev[di];
        const uint32_t n_local = bsh::shard_blocks(n_blocks, di, nd);
        s.shard.n_blocks = n_local;
        // this device's sections in file order
        std::vector<uint32_t> idx;
        for (uint32_t lb = 0; lb < n_local; ++lb) idx.push_back(lb * nd + di);
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return sec_begin[a] < sec_begin[b]; });
        uint64_t cursor = 0, prev_end = 0;
        for (uint32_t b : idx) {
            const uint64_t len = sec_end[b] - sec_begin[b];
            if (len == 0) continue;                                   // block without a section: nil filters, status 0
            if (sec_begin[b] < prev_end) return fail(BSG_E_INVALID, "section %u overlaps its predecessor", b);
            prev_end = sec_end[b];
            // a section's words need fewer bytes than the section; three filters re-aligned to 128 bytes need <= 3 x 120 more
            const uint64_t cap_words = ((len + 3 * 128) / 8 + kAlignWords - 1) / kAlignWords * kAlignWords;
            s.slots.push_back(bsg::SectionSlot{sec_begin[b] - st->base, cursor, (uint32_t)len, (uint32_t)cap_words, b / nd,
                                               len >= 5 ? bsg::crc_init_image(len - 4, crc_consts().x2n) : 0u});
            s.ends.push_back(sec_end[b] - st->base);
            s.global_block.push_back(b);
            cursor += cap_words;
        }
        s.decoded.assign(s.slots.size(), 0);
        s.shard.n_words = cursor + kAlignWords;
    }
    for (uint32_t di = 0; di < nd; ++di) {
        Device &d = *ctx->devs[di];
        StreamDev &s = st->dev[di];
        const uint32_t n_local = s.shard.n_blocks;
        std::unique_lock<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) { lk.unlock(); free_stream(ctx, *st, false); return rc; }
        hipError_t e = hipSuccess;
        if (!d.d_crc) {
            e = hipMalloc(reinterpret_cast<void **>(&d.d_crc), sizeof(bsg::CrcConsts));
            if (e == hipSuccess) e = hipMemcpyAsync(d.d_crc, &crc_consts(), sizeof(bsg::CrcConsts), hipMemcpyHostToDevice, d.stream);
        }
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.shard.d_words), s.shard.n_words * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.shard.d_desc), std::max<size_t>(n_local, 1) * 3 * sizeof(DevDesc));
        if (e == hipSuccess) e = hipMemsetAsync(s.shard.d_desc, 0, std::max<size_t>(n_local, 1) * 3 * sizeof(DevDesc), d.stream);
        if (e == hipSuccess) e = d.pool.alloc(reinterpret_cast<void **>(&s.d_status), std::max<size_t>(n_local, 1) * 4);
        if (e == hipSuccess) e = hipMemsetAsync(s.d_status, 0, std::max<size_t>(n_local, 1) * 4, d.stream);
        if (e == hipSuccess && !s.slots.empty()) {
            e = d.pool.alloc(reinterpret_cast<void **>(&s.d_region), st->span + 64);
            if (e == hipSuccess) e = d.pool.alloc(reinterpret_cast<void **>(&s.d_slots), s.slots.size() * sizeof(bsg::SectionSlot));
            if (e == hipSuccess) e = hipMemcpyAsync(s.d_slots, s.slots.data(), s.slots.size() * sizeof(bsg::SectionSlot), hipMemcpyHostToDevice, d.stream);
            if (e == hipSuccess) e = d.pool.alloc(reinterpret_cast<void **>(&s.d_crc_acc), s.slots.size() * 8);
            if (e == hipSuccess) e = hipMemsetAsync(s.d_crc_acc, 0, s.slots.size() * 8, d.stream);
            for (int i = 0; i < 2 && e == hipSuccess; ++i) {
                if (!d.idle_staging.empty()) { s.staging[i] = d.idle_staging.back(); d.idle_staging.pop_back(); }
                else e = hipHostMalloc(reinterpret_cast<void **>(&s.staging[i]), kStreamChunk, hipHostMallocDefault);
            }
            if (e == hipSuccess && !d.idle_kits.empty()) {            // copy stream + events of a finished stream
                const Device::StreamKit k = d.idle_kits.back();
                d.idle_kits.pop_back();
                s.copy = k.copy; s.copied = k.copied; s.staged_free[0] = k.staged_free[0]; s.staged_free[1] = k.staged_free[1];
            } else {
                for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&s.staged_free[i], hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
                if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.copy, hipStreamNonBlocking);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);      // slot table / zeroed descriptors in place before any decode
        if (e != hipSuccess) {
            const int32_t rc = fail(e == hipErrorOutOfMemory ? BSG_E_NOMEM : BSG_E_HIP, "arena stream: %s", hipGetErrorString(e));
            lk.unlock();
            free_stream(ctx, *st, false);
            return rc;
        }
    }
    out = st;
    return BSG_OK;
}

int32_t stream_finish(bsg_ctx *ctx, ArenaStream &st, int32_t *out_status, uint64_t *out_arena_id)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    for (uint32_t b = 0; b < st.n_blocks; ++b) out_status[b] = 0;
    for (uint32_t di = 0; di < nd; ++di) {
        Device &d = *ctx->devs[di];
        StreamDev &s = st.dev[di];
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) return rc;
        if (s.copy) HIP_TRY(hipStreamSynchronize(s.copy));
        HIP_TRY(hipStreamSynchronize(d.stream));
        const uint32_t n_local = s.shard.n_blocks;
        std::vector<int32_t> status(std::max(n_local, 1u), 0);
        std::vector<DevDesc> dd((size_t)std::max(n_local, 1u) * 3);
        HIP_TRY(hipMemcpy(status.data(), s.d_status, (size_t)std::max(n_local, 1u) * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dd.data(), s.shard.d_desc, dd.size() * sizeof(DevDesc), hipMemcpyDeviceToHost));
        for (uint32_t lb = 0; lb < n_local; ++lb) out_status[lb * nd + di] = status[lb];
        for (size_t i = 0; i < s.slots.size(); ++i)
            if (!s.decoded[i] && s.slots[i].len != 0) out_status[s.global_block[i]] = kSectionUnread;
        ArenaShard &sh = s.shard;
        for (uint32_t lb = 0; lb < n_local; ++lb)
            for (uint32_t c = 0; c < 3; ++c) sh.add_filter(c, dd[(size_t)lb * 3 + c].m, dd[(size_t)lb * 3 + c].k);
        float ms = 0.f;
        for (auto &t : s.timers) { float x = 0.f; if (hipEventElapsedTime(&x, t.first, t.second) == hipSuccess) ms += x; }
        { std::lock_guard<std::shared_mutex> lk2(ctx->mu); ctx->last_decode_ms = di == 0 ? ms : std::max(ctx->last_decode_ms, ms); }
        st.arena->shards[di] = sh;
    }
    for (uint32_t di = 0; di < nd; ++di) {
        std::lock_guard<std::mutex> lk(ctx->devs[di]->mu);
        free_stream_dev(*ctx->devs[di], st.dev[di], true);
    }
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    const uint64_t id = ctx->next_id++;
    ctx->arenas[id] = st.arena;
    *out_arena_id = id;
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_arena_stream_begin(bsg_ctx *ctx, const uint64_t *sec_begin, const uint64_t *sec_end, uint32_t n_blocks, uint64_t *out_stream_id)
{
    BSG_ENTER(ctx);
    if (!out_stream_id || (n_blocks && (!sec_begin || !sec_end))) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<ArenaStream> st;
    if (int32_t rc = stream_begin(ctx, sec_begin, sec_end, n_blocks, st)) return rc;
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    const uint64_t id = ctx->next_id++;
    ctx->streams[id] = st;
    *out_stream_id = id;
    return BSG_OK;
}

int32_t bsg_arena_stream_append(bsg_ctx *ctx, uint64_t stream_id, uint64_t file_offset, const uint8_t *bytes, uint64_t len)
{
    BSG_ENTER(ctx);
    if (len && !bytes) return fail(BSG_E_INVALID, "bytes is null");
    std::shared_ptr<ArenaStream> st;
    if (int32_t rc = get_stream(ctx, stream_id, st)) return rc;
    return stream_append(ctx, *st, file_offset, bytes, len);
}

int32_t bsg_arena_stream_finish(bsg_ctx *ctx, uint64_t stream_id, int32_t *out_status, uint64_t *out_arena_id)
{
    BSG_ENTER(ctx);
    if (!out_arena_id) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<ArenaStream> st;
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        auto it = ctx->streams.find(stream_id);
        if (it == ctx->streams.end()) return fail(BSG_E_NOTFOUND, "unknown arena stream id %llu", (unsigned long long)stream_id);
        st = it->second;
        ctx->streams.erase(it);
    }
    if (st->n_blocks && !out_status) { free_stream(ctx, *st, false); return fail(BSG_E_INVALID, "out_status is null"); }
    const int32_t rc = stream_finish(ctx, *st, out_status, out_arena_id);
    if (rc) free_stream(ctx, *st, false);
    return rc;
}

int32_t bsg_arena_stream_abort(bsg_ctx *ctx, uint64_t stream_id)
{
    BSG_ENTER(ctx);
    std::shared_ptr<ArenaStream> st;
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        auto it = ctx->streams.find(stream_id);
        if (it == ctx->streams.end()) return fail(BSG_E_NOTFOUND, "unknown arena stream id %llu", (unsigned long long)stream_id);
        st = it->second;
        ctx->streams.erase(it);
    }
    free_stream(ctx, *st, false);
    return BSG_OK;
}

// Arena straight from the on-disk bytes: the whole region through the streaming path (copy of piece i + 1 beside the decode of piece i).
int32_t bsg_arena_load_sections(bsg_ctx *ctx, const uint8_t *region, uint64_t region_len, const uint64_t *sec_off, uint32_t n_blocks,
                                int32_t *out_status, uint64_t *out_arena_id)
{
    BSG_ENTER(ctx);
    if (!out_arena_id || (n_blocks && (!sec_off || !out_status))) return fail(BSG_E_INVALID, "null argument");
    if (region_len && !region) return fail(BSG_E_INVALID, "region is null");
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (sec_off[b + 1] < sec_off[b] || sec_off[b + 1] > region_len) return fail(BSG_E_INVALID, "sec_off not monotone / outside region at %u", b);
    std::shared_ptr<ArenaStream> st;
    if (int32_t rc = stream_begin(ctx, sec_off, sec_off + (n_blocks ? 1 : 0), n_blocks, st)) return rc;
    int32_t rc = BSG_OK;
    // The whole region is here already, so the pieces only set how much decode work one launch gets and how soon the
    // first launch can start behind the copy: a quarter of the region each (one 4 MiB piece holds ~60 sections = 60
    // workgroups on 256 CUs: 17 such launches took 870 us for 70 MB, four launches of ~250 take 90 us).
    const uint64_t pieces = ctx->load_pieces;
    const uint64_t piece = pieces <= 1 ? std::max<uint64_t>(region_len, 1)
                                       : std::min<uint64_t>(std::max<uint64_t>((region_len / pieces + kStreamChunk - 1) / kStreamChunk * kStreamChunk, kStreamChunk), 64ull << 20);
    for (uint64_t o = 0; o < region_len && !rc; o += piece) rc = stream_append(ctx, *st, o, region + o, std::min(piece, region_len - o), true);
    if (!rc) rc = stream_finish(ctx, *st, out_status, out_arena_id);
    if (rc) free_stream(ctx, *st, false);
    return rc;
}

}  // extern "C"
