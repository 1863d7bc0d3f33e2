// probe_api.inc — the read path behind the C-ABI (included by bloomgpu.hip): query batches (bsg_batch_create: term tables,
// lowered programs, composite batches beyond one launch's limits), the launch groups and their kernels' arguments, probe_arenas
// (bsg_probe_batch / bsg_probe_many / _dev / _rows: k_probe_terms(_many) + k_eval_programs per group of arenas, the fused and
// folded variants, the one-dispatch path, survivors out by copy stream or as rows written by the device), bsg_probe and the
// one-call bsg_query (k_query_direct).  evaluateBloom{Filters,Expression,Condition} and the block loop of the reference:
// query_exec.go:75-159, 572-615.
namespace {

// The tables one launch-sized batch leaves on a device: SoA term hashes, lane-interleaved lowered programs per 256-query chunk,
// each chunk's length and verdict-word list.
struct BatchTables {
    std::vector<uint64_t> th;
    std::vector<uint32_t> packed, chunk_len, cw_cnt, cw;
    // one buffer layout for all five (each table on a 256-byte boundary): what upload_packed copies and BatchDev points into
    size_t off_th = 0, off_prog = 0, off_len = 0, off_cnt = 0, off_cw = 0, total = 0;
    void layout()
    {
        auto up = [](size_t x) { return (x + 255) / 256 * 256; };
        off_th = 0;
        off_prog = up(th.size() * 8);
        off_len = off_prog + up(std::max<size_t>(packed.size(), 1) * 4);
        off_cnt = off_len + up(chunk_len.size() * 4);
        off_cw = off_cnt + up(cw_cnt.size() * 4);
        total = off_cw + up(std::max<size_t>(cw.size(), 1) * 4);
    }
    void pack_into(uint8_t *dst) const
    {
        memcpy(dst + off_th, th.data(), th.size() * 8);
        if (!packed.empty()) memcpy(dst + off_prog, packed.data(), packed.size() * 4);
        memcpy(dst + off_len, chunk_len.data(), chunk_len.size() * 4);
        memcpy(dst + off_cnt, cw_cnt.data(), cw_cnt.size() * 4);
        if (!cw.empty()) memcpy(dst + off_cw, cw.data(), cw.size() * 4);
    }
    BatchDev dev_at(uint8_t *base) const
    {
        BatchDev bd;
        bd.d_th = reinterpret_cast<uint64_t *>(base + off_th);
        bd.d_prog = reinterpret_cast<uint32_t *>(base + off_prog);
        bd.d_chunk_len = reinterpret_cast<uint32_t *>(base + off_len);
        bd.d_cw_cnt = reinterpret_cast<uint32_t *>(base + off_cnt);
        bd.d_cw = reinterpret_cast<uint32_t *>(base + off_cw);
        return bd;
    }
};

// The host half of a launch-sized batch: term layout (grouped by kind, 64-term segments), the programs — already LOWERED to the
// binary postfix, TERM arguments = indices into `terms` — packed per 256-query chunk.  Fills B's geometry and T; nothing touches a
// device.  *too_big: the failure (BSG_E_UNSUPPORTED) is one a smaller run of queries may not have.
int32_t plan_batch_tables(const bsg_term *terms, uint32_t n_terms, const std::vector<std::vector<uint32_t>> &lowered, uint32_t max_depth,
                          Batch &B, BatchTables &T, bool *too_big)
{
    *too_big = false;
    const uint32_t n_queries = (uint32_t)lowered.size();
    B.n_queries = n_queries;
    B.max_depth = std::max(max_depth, 1u);
    // group terms by kind; each kind's segment starts on a 64-term boundary
    uint32_t count[3] = {0, 0, 0};
    for (uint32_t t = 0; t < n_terms; ++t) {
        if (terms[t].kind > 2) return fail(BSG_E_INVALID, "term %u has unknown kind %u", t, terms[t].kind);
        count[terms[t].kind]++;
    }
    uint32_t begin_of_kind[3] = {0, 0, 0};
    uint32_t cursor = 0;
    for (uint32_t c = 0; c < 3; ++c) {
        if (count[c] == 0) continue;
        B.kind[B.n_kinds] = c;
        B.term_begin[B.n_kinds] = cursor;
        B.term_count[B.n_kinds] = count[c];
        begin_of_kind[c] = cursor;
        cursor += (count[c] + 63) / 64 * 64;
        B.n_kinds++;
    }
    B.Tp = cursor;
    B.Wt = cursor / 64;
    std::vector<uint32_t> term_pos(n_terms);
    T.th.assign((size_t)4 * std::max(B.Tp, 1u), 0);
    uint32_t fill[3] = {0, 0, 0};
    for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t c = terms[t].kind;
        const uint32_t pos = begin_of_kind[c] + fill[c]++;
        term_pos[t] = pos;
        for (int j = 0; j < 4; ++j) T.th[(size_t)j * B.Tp + pos] = terms[t].h[j];
    }
    // pack per 256-query chunk in lane-interleaved (coalesced) order with ONE stride for all chunks (Lmax ops, NOP padded) and one
    // stride for the per-chunk verdict-word lists (max_cw)
    B.n_chunks = (n_queries + bsg::kEvalThreads - 1) / bsg::kEvalThreads;
    for (uint32_t q = 0; q < n_queries; ++q) B.Lmax = std::max<uint32_t>(B.Lmax, (uint32_t)lowered[q].size());
    B.identity_cw = B.Wt >= 1 && B.Wt <= 8;
    for (uint32_t y = 0; y < B.n_kinds; ++y) if ((B.term_count[y] + 63) / 64 > bsg::kParallelKMaxWords) B.many_terms = true;
    T.chunk_len.assign(std::max(B.n_chunks, 1u), 0);
    T.cw_cnt.assign(std::max(B.n_chunks, 1u), 0);
    std::vector<std::vector<uint32_t>> chunk_words(B.n_chunks);
    for (uint32_t c = 0; c < B.n_chunks; ++c) {
        const uint32_t q0 = c * bsg::kEvalThreads;
        const uint32_t nq = std::min<uint32_t>(bsg::kEvalThreads, n_queries - q0);
        std::vector<uint32_t> &words = chunk_words[c];   // verdict words this chunk references -> slots
        for (uint32_t i = 0; i < nq; ++i) {
            T.chunk_len[c] = std::max<uint32_t>(T.chunk_len[c], (uint32_t)lowered[q0 + i].size());
            if (!B.identity_cw)
                for (uint32_t op : lowered[q0 + i])
                    if ((op >> 28) == 0u) words.push_back(term_pos[op & 0x0FFFFFFFu] >> 6);
        }
        if (B.identity_cw) { words.resize(B.Wt); for (uint32_t w = 0; w < B.Wt; ++w) words[w] = w; }
        else {
            std::sort(words.begin(), words.end());
            words.erase(std::unique(words.begin(), words.end()), words.end());
        }
        T.cw_cnt[c] = (uint32_t)words.size();
        B.max_cw = std::max<uint32_t>(B.max_cw, (uint32_t)words.size());
    }
    T.packed.assign((size_t)std::max(B.n_chunks, 1u) * B.Lmax * bsg::kEvalThreads, 7u << 28);
    T.cw.assign((size_t)std::max(B.n_chunks, 1u) * B.max_cw, 0);
    for (uint32_t c = 0; c < B.n_chunks; ++c) {
        const uint32_t q0 = c * bsg::kEvalThreads;
        const uint32_t nq = std::min<uint32_t>(bsg::kEvalThreads, n_queries - q0);
        const std::vector<uint32_t> &words = chunk_words[c];
        std::copy(words.begin(), words.end(), T.cw.begin() + (size_t)c * B.max_cw);
        for (uint32_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < lowered[q0 + i].size(); ++j) {
                uint32_t op = lowered[q0 + i][j];
                if ((op >> 28) == 0u) {   // TERM args become slot * 64 + bit
                    const uint32_t pos = term_pos[op & 0x0FFFFFFFu];
                    const uint32_t slot = B.identity_cw ? (pos >> 6) : (uint32_t)(std::lower_bound(words.begin(), words.end(), pos >> 6) - words.begin());
                    op = slot * 64 + (pos & 63);
                }
                T.packed[((size_t)c * B.Lmax + j) * bsg::kEvalThreads + i] = op;
            }
    }
    if (T.packed.size() > (1ull << 30)) {
        *too_big = true;
        return fail(BSG_E_UNSUPPORTED, "padded program table of %zu ops is too large for one launch", T.packed.size());
    }
    const size_t lds_need = ((size_t)B.max_cw * 64 + (size_t)B.max_depth * bsg::kEvalThreads) * 8;
    if (lds_need > 64 * 1024) {
        *too_big = true;
        return fail(BSG_E_UNSUPPORTED, "a 256-query chunk needs %zu B of LDS (%u verdict words, stack depth %u)", lds_need,
                    B.max_cw, B.max_depth);
    }
    {
        // k_probe_terms keeps per-kind verdict words + wave queues in LDS beside the bitset image
        uint32_t max_tw = 0;
        for (uint32_t y = 0; y < B.n_kinds; ++y) max_tw = std::max(max_tw, (B.term_count[y] + 63) / 64);
        if (bsg::probe_lds_head_bytes(max_tw) > 48 * 1024) {
            *too_big = true;
            return fail(BSG_E_UNSUPPORTED, "%u distinct terms of one kind exceed what one probe launch holds", max_tw * 64);
        }
    }
    T.layout();
    return BSG_OK;
}

// One batch that fits one launch's limits.  *too_big: the failure (BSG_E_UNSUPPORTED) is one a smaller run of queries may not have.
int32_t create_simple_batch(bsg_ctx *ctx, const bsg_term *terms, uint32_t n_terms, const uint32_t *prog_ops, const uint32_t *prog_off,
                            uint32_t n_queries, std::shared_ptr<Batch> &out, bool *too_big)
{
    *too_big = false;
    auto batch = std::make_shared<Batch>();
    Batch &B = *batch;
    std::vector<uint32_t> identity(n_terms);
    for (uint32_t t = 0; t < n_terms; ++t) identity[t] = t;
    for (uint32_t t = 0; t < n_terms; ++t)
        if (terms[t].kind > 2) return fail(BSG_E_INVALID, "term %u has unknown kind %u", t, terms[t].kind);
    std::vector<std::vector<uint32_t>> lowered(n_queries);
    uint32_t max_depth = 1;
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
        const uint32_t n_ops = prog_off[q + 1] - prog_off[q];
        if (n_ops && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
        uint32_t depth = 1;
        if (int32_t rc = lower_program(prog_ops + prog_off[q], n_ops, n_terms, identity, lowered[q], depth)) return rc;
        max_depth = std::max(max_depth, depth);
    }
    BatchTables T;
    if (int32_t rc = plan_batch_tables(terms, n_terms, lowered, max_depth, B, T, too_big)) return rc;
    // one allocation and one copy per device: the five tables packed behind each other (BatchDev::d_th owns the block)
    std::vector<uint8_t> packed_host(T.total, 0);
    T.pack_into(packed_host.data());
    B.dev.resize(ctx->devs.size());
    for (size_t di = 0; di < ctx->devs.size(); ++di) {
        Device &d = *ctx->devs[di];
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) { free_batch(ctx, B); return rc; }
        uint8_t *base = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), T.total);
        if (e == hipSuccess) {
            B.dev[di] = T.dev_at(base);
            e = hipMemcpyAsync(base, packed_host.data(), T.total, hipMemcpyHostToDevice, d.stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            free_batch(ctx, B);
            return fail(e == hipErrorOutOfMemory ? BSG_E_NOMEM : BSG_E_HIP, "batch upload failed: %s", hipGetErrorString(e));
        }
    }
    out = batch;
    return BSG_OK;
}

// A batch of any size: one simple batch when it fits a launch, otherwise runs of queries (halved until they fit), each with the
// terms its own queries reference.  A single query beyond the limits stays unsupported.
int32_t create_batch_tree(bsg_ctx *ctx, const bsg_term *terms, uint32_t n_terms, const uint32_t *prog_ops, const uint32_t *prog_off,
                          uint32_t q0, uint32_t q1, std::vector<std::shared_ptr<Batch>> &subs, std::vector<uint32_t> &sub_q0)
{
    // the run's own terms and programs (term indices renumbered densely in order of first use)
    std::vector<uint32_t> remap(n_terms, 0xFFFFFFFFu), ops, off{0};
    std::vector<bsg_term> used;
    for (uint32_t q = q0; q < q1; ++q) {
        for (uint32_t j = prog_off[q]; j < prog_off[q + 1]; ++j) {
            uint32_t op = prog_ops[j];
            if ((op >> 28) == BSG_OP_TERM) {
                const uint32_t t = op & 0x0FFFFFFFu;
                if (t >= n_terms) return fail(BSG_E_INVALID, "program references term %u of %u", t, n_terms);
                if (remap[t] == 0xFFFFFFFFu) { remap[t] = (uint32_t)used.size(); used.push_back(terms[t]); }
                op = BSG_OP(BSG_OP_TERM, remap[t]);
            }
            ops.push_back(op);
        }
        off.push_back((uint32_t)ops.size());
    }
    std::shared_ptr<Batch> b;
    bool too_big = false;
    const int32_t rc = create_simple_batch(ctx, used.data(), (uint32_t)used.size(), ops.data(), off.data(), q1 - q0, b, &too_big);
    if (rc == BSG_OK) { subs.push_back(b); sub_q0.push_back(q0); return BSG_OK; }
    if (!too_big || q1 - q0 <= 1) return rc;
    // halves on 256-query (chunk) boundaries where the run is long enough
    uint32_t mid = q0 + (q1 - q0) / 2;
    if (q1 - q0 > 2 * bsg::kEvalThreads) mid = q0 + (mid - q0 + bsg::kEvalThreads - 1) / bsg::kEvalThreads * bsg::kEvalThreads;
    if (int32_t rc2 = create_batch_tree(ctx, terms, n_terms, prog_ops, prog_off, q0, mid, subs, sub_q0)) return rc2;
    return create_batch_tree(ctx, terms, n_terms, prog_ops, prog_off, mid, q1, subs, sub_q0);
}

}  // namespace

extern "C" {

int32_t bsg_batch_create(bsg_ctx *ctx, const bsg_term *terms, uint32_t n_terms, const uint32_t *prog_ops,
                         const uint32_t *prog_off, uint32_t n_queries, uint64_t *out_batch_id)
{
    BSG_ENTER(ctx);
    if (!ctx || !out_batch_id) return fail(BSG_E_INVALID, "null argument");
    if (n_terms && !terms) return fail(BSG_E_INVALID, "terms is null");
    if (n_queries && !prog_off) return fail(BSG_E_INVALID, "prog_off is null");
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
        if (prog_off[q + 1] > prog_off[q] && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    }
    std::shared_ptr<Batch> batch;
    bool too_big = false;
    int32_t rc = create_simple_batch(ctx, terms, n_terms, prog_ops, prog_off, n_queries, batch, &too_big);
    if (rc && too_big && n_queries > 1) {
        // beyond one launch: a composite of runs of queries (the caller sees one batch; the evaluator it replaces has no limit)
        auto comp = std::make_shared<Batch>();
        comp->n_queries = n_queries;
        rc = create_batch_tree(ctx, terms, n_terms, prog_ops, prog_off, 0, n_queries, comp->subs, comp->sub_q0);
        if (rc) { const std::string saved = g_err; free_batch(ctx, *comp); return fail(rc, "%s", saved.c_str()); }
        batch = comp;
    }
    if (rc) return rc;
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    const uint64_t id = ctx->next_id++;
    ctx->batches[id] = batch;
    *out_batch_id = id;
    return BSG_OK;
}

int32_t bsg_batch_free(bsg_ctx *ctx, uint64_t batch_id)
{
    BSG_ENTER(ctx);
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    std::shared_ptr<Batch> b;
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        auto it = ctx->batches.find(batch_id);
        if (it == ctx->batches.end()) return fail(BSG_E_NOTFOUND, "unknown batch id %llu", (unsigned long long)batch_id);
        b = it->second;
        ctx->batches.erase(it);
    }
    for (auto &dp : ctx->devs) {
        std::lock_guard<std::mutex> lk(dp->mu);
        (void)hipSetDevice(dp->id);
        (void)hipStreamSynchronize(dp->stream);
    }
    free_batch(ctx, *b);
    return BSG_OK;
}

}  // extern "C"

namespace {

int32_t take_events(bsg_ctx *ctx, Device &d, EventTriple &ev)
{
    if (d.pending.size() >= 4096) if (int32_t rc = drain_timing(ctx, d)) return rc;
    if (!d.free_events.empty()) { ev = d.free_events.back(); d.free_events.pop_back(); }
    else {
        HIP_TRY(hipEventCreate(&ev.k1s)); HIP_TRY(hipEventCreate(&ev.k1e));
        HIP_TRY(hipEventCreate(&ev.k2s)); HIP_TRY(hipEventCreate(&ev.k2e));
        ev.ran = nullptr;
    }
    ev.bytes = 0;
    ev.counted = false;
    ev.has_k1 = ev.has_k2 = ev.fused = ev.folded = false;
    ev.n_arenas = 0;
    return BSG_OK;
}

// A launch group: the shards (on one device) of up to kMaxGroupArenas arenas, probed by ONE dispatch — the plan's figures
// (host/probe_plan.hpp: index, v_words, out_words, max_blocks, max_G, total_G) and the shards they stand for.
struct Group : bsh::GroupPlan {
    std::vector<const ArenaShard *> shards;
};

// the group's arena records from position i0 on (at most `cap` of them); g_prefix counts from the group's first arena
void fill_refs(const Group &g, bsg::ArenaRef *refs, size_t i0 = 0, size_t cap = ~size_t(0))
{
    uint32_t gp = 0;
    for (size_t i = 0; i < g.shards.size() && i < i0 + cap; ++i) {
        const ArenaShard &s = *g.shards[i];
        if (i >= i0) refs[i - i0] = bsg::ArenaRef{s.d_words, s.d_desc, s.n_blocks, gp};
        gp += (s.n_blocks + 63) / 64;
    }
}

void group_add(Group &g, uint32_t n_queries, uint32_t Wt, const ArenaShard &s, uint32_t idx)
{
    g.add(idx, s.n_blocks, n_queries, Wt);
    g.shards.push_back(&s);
}

// block counts as the plan takes them (i -> blocks): of the arenas, and of their shards on device di
struct ArenaBlocks {
    const std::vector<std::shared_ptr<Arena>> &arenas;
    uint32_t operator()(uint32_t i) const { return arenas[i]->n_blocks; }
};

struct ShardBlocks {
    const std::vector<std::shared_ptr<Arena>> &arenas;
    uint32_t di;
    uint32_t operator()(uint32_t i) const { return arenas[i]->shards[di].n_blocks; }
};

// The arena records of a group for k_probe_terms(_many) / k_eval_programs: in the kernel arguments up to kMaxGroupArenas, else
// uploaded into the scratch slot's device table in front of the dispatch (same stream: ordered before it, and after the
// previous user of the slot).  *ext = nullptr or the device table.  force_ext: the device table whatever the group's size (a group
// probed in chunks, DeviceRun::pipeline_chunked: both roles of k_gather_fused index the group's records by arena).
int32_t group_table(Device &d, const Group &g, bsg::ArenaTable<bsg::kMaxGroupArenas> &t, const bsg::ArenaRef **ext, bool force_ext = false)
{
    *ext = nullptr;
    const size_t n = g.shards.size();
    if (n <= bsg::kMaxGroupArenas && !force_ext) { fill_refs(g, t.ar); return BSG_OK; }
    // A table in device memory is a pure function of its records, and hosts probe the same candidate files again and again: the
    // device keeps the last few tables it wrote (round 5), so a group that was probed before costs no k_write_arena_table dispatches
    // — two serial ~5 us dispatches in front of the stream for the 200 shards a rank holds of 20 steps x 10 files at N = 8.
    std::vector<bsg::ArenaRef> refs(n);
    fill_refs(g, refs.data());
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
    for (const auto &r : refs) { h = (h ^ (uint64_t)(uintptr_t)r.words) * 0x100000001B3ull; h = (h ^ (uint64_t)(uintptr_t)r.desc) * 0x100000001B3ull; h = (h ^ r.n_blocks) * 0x100000001B3ull; }
    for (auto &c : d.table_cache)
        if (c.hash == h && c.refs.size() == n && memcmp(c.refs.data(), refs.data(), n * sizeof(bsg::ArenaRef)) == 0) {
            c.last_use = ++d.table_tick;
            *ext = c.buf.p;
            return BSG_OK;
        }
    Device::TableEntry *e = nullptr;
    if (d.table_cache.size() < Device::kTableCache) { d.table_cache.emplace_back(); e = &d.table_cache.back(); }
    else for (auto &c : d.table_cache) if (!e || c.last_use < e->last_use) e = &c;      // (reused behind its last reader: same in-order stream)
    HIP_TRY(e->buf.reserve(n));
    e->hash = 0; e->refs.clear();
    // the records travel in the kernel arguments of k_write_arena_table, 128 per launch: captured at enqueue time, so an
    // asynchronous call leaves no host buffer behind for a later copy to read
    for (size_t i0 = 0; i0 < n; i0 += bsg::kMaxGroupArenas) {
        const size_t m = std::min<size_t>(bsg::kMaxGroupArenas, n - i0);
        memcpy(t.ar, refs.data() + i0, m * sizeof(bsg::ArenaRef));
        hipLaunchKernelGGL(bsg::k_write_arena_table, dim3(1), dim3(bsg::kMaxGroupArenas), 0, d.stream, e->buf.p + i0, t, (uint32_t)m);
        HIP_TRY(hipGetLastError());
    }
    e->hash = h; e->refs = std::move(refs); e->last_use = ++d.table_tick;
    *ext = e->buf.p;
    return BSG_OK;
}

// K1 arguments: stream every referenced bitset of the group once, one verdict word per (block, 64 terms) into V[slot].
int32_t make_probe_args(bsg_ctx *ctx, Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint32_t slot, EventTriple *ev,
                        bsg::ProbeArgs &a, uint32_t &lds_bytes)
{
    HIP_TRY(d.V[slot].reserve(std::max<uint64_t>(g.v_words, 1)));
    a = bsg::ProbeArgs{};
    a.th = bd.d_th; a.V = d.V[slot].p;
    a.Tp = B.Tp; a.Wt = B.Wt;
    a.n_arenas = (uint32_t)g.shards.size();
    a.max_blocks = g.max_blocks;
    a.gather_cost = ctx->gather_cost;
    uint32_t max_tw = 0;
    for (uint32_t y = 0; y < B.n_kinds; ++y) max_tw = std::max(max_tw, (B.term_count[y] + 63) / 64);
    const size_t head = bsg::probe_lds_head_bytes(max_tw);
    // staged-filter cap for this launch: what is left of the LDS budget after the head
    const uint64_t cap_words = head + 32 < kLdsBudget ? (kLdsBudget - head) / 16 * 2 : 0;
    a.lds_cap_words = (uint32_t)std::min<uint64_t>(kLdsCapWords, cap_words);
    uint64_t lds_words = 2;
    for (uint32_t y = 0; y < B.n_kinds; ++y) {
        a.kind[y] = B.kind[y]; a.term_begin[y] = B.term_begin[y]; a.term_count[y] = B.term_count[y];
        for (const ArenaShard *s : g.shards) {
            lds_words = std::max(lds_words, std::min<uint64_t>(s->max_staged_words[B.kind[y]], a.lds_cap_words));
            if (ev) ev->bytes += s->sum_words[B.kind[y]] * 8;
        }
    }
    if (ev) ev->n_arenas = a.n_arenas;
    lds_words = (lds_words + 1) / 2 * 2;
    a.lds_image_bytes = (uint32_t)(lds_words * 8);
    a.compact_rounds = ctx->compact_rounds;
    lds_bytes = (uint32_t)(head + lds_words * 8);
    return BSG_OK;
}

int32_t make_eval_args(Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint32_t slot, bsg::EvalArgs &a)
{
    HIP_TRY(d.out[slot].reserve(std::max<uint64_t>(g.out_words, 1)));
    a = bsg::EvalArgs{};
    a.V = d.V[slot].p; a.prog = bd.d_prog; a.chunk_len = bd.d_chunk_len;
    a.out = d.out[slot].p; a.Wt = B.Wt; a.n_queries = B.n_queries;
    a.cw_cnt = bd.d_cw_cnt; a.cw = bd.d_cw; a.max_cw = B.max_cw; a.Lmax = B.Lmax; a.identity_cw = B.identity_cw ? 1u : 0u;
    a.n_arenas = (uint32_t)g.shards.size();
    a.max_G = g.max_G;
    return BSG_OK;
}

// Small launches keep one block group per eval workgroup (latency); large ones tile kEvalGroupTile groups so a
// query's survivor words leave as one 32-byte store instead of four strided 8-byte stores.
// (A 32-arena group of 1 000-block arenas with one group per workgroup wrote 66.7 MB for 16.8 MB of survivors: 8-byte
// stores at a 128-byte stride cost a 32-byte sector each.)
uint32_t eval_tile_for(const Group &g)
{
    static const char *force = getenv("BSG_LAB_EVAL_TILE");   // lab only
    if (force) return std::max(1, atoi(force));
    if (!(g.max_G >= 64 || g.total_G >= 64)) return 1u;
    return g.max_G <= 2 ? 2u : bsg::kEvalGroupTile;          // (many small shards — a file's 125 blocks on one of 8 GPUs — take tiles of 2 groups)
}

// What bsh::launch_gathers / bsh::gathered_bytes take of a group (or of a chunk of one): per referenced kind the filters' words, the
// part beyond the LDS budget, the batch's terms and the largest k; -> the blocks of the group.
uint64_t gather_kinds(const Group &g, const Batch &B, bsh::GatherKind *gk)
{
    uint64_t group_blocks = 0;
    for (const ArenaShard *s : g.shards) group_blocks += s->n_blocks;
    for (uint32_t y = 0; y < B.n_kinds; ++y) {
        gk[y] = bsh::GatherKind{0, 0, B.term_count[y], 0};
        for (const ArenaShard *s : g.shards) {
            gk[y].sum_words += s->sum_words[B.kind[y]];
            gk[y].unstaged_words += s->sum_unstaged_words[B.kind[y]];
            gk[y].max_k = std::max(gk[y].max_k, s->max_k[B.kind[y]]);
        }
    }
    return group_blocks;
}

// dynamic LDS the gather kernels are launched with although they use none: it caps their workgroups per CU (bsh::gather_lds_pad;
// bsg_set_lab key 28, 0 = the planner's rule)
uint32_t gather_pad(const bsg_ctx *ctx)
{
    return bsh::gather_lds_pad(ctx->gather_wgs_per_cu ? ctx->gather_wgs_per_cu : bsh::kGatherWorkgroupsPerCu);
}

bool group_gathers(const bsg_ctx *ctx, const Group &g, const Batch &B)
{
    bsh::GatherKind gk[3];
    const uint64_t group_blocks = gather_kinds(g, B, gk);
    return B.n_kinds > 0 && ctx->gather_kernel && bsh::launch_gathers(gk, B.n_kinds, group_blocks, B.many_terms, ctx->gather_cost);
}

// bsg_timing's stream_bytes for a gathered launch (ev->bytes holds the bitsets' bytes, make_probe_args): not the bitsets (it does not
// stream them) but the 128-byte lines its bit tests are expected to touch (what FETCH_SIZE shows) — a roofline fraction formed from
// it stays one.  Here: bsh::gathered_bytes, every location of every term; the kernel skips the later locations of a term absent from
// a block, so it counts the tests it executes into the triple's counters (gather_counters, before the launch) and drain_timing
// puts bsh::gathered_bytes_tests of them in its place.
void gathered_timing(EventTriple &ev, const Batch &B, const bsh::GatherKind *gk, uint64_t group_blocks)
{
    ev.n_gk = B.n_kinds;
    ev.gk_blocks = group_blocks;
    ev.gk_model = 0;
    for (uint32_t y = 0; y < B.n_kinds; ++y) {
        ev.gk[y] = gk[y];
        ev.bytes -= gk[y].sum_words * 8;
        ev.gk_model += bsh::gathered_bytes(gk[y], group_blocks);
    }
    ev.bytes += ev.gk_model;
    ev.counted = ev.ran != nullptr;
    ev.has_k1 = true;
}

// the counters a timestamped gathered launch sums its executed bit tests into, zeroed on the stream ahead of it (nullptr: not timestamped)
int32_t gather_counters(Device &d, EventTriple *ev, uint64_t **ran)
{
    *ran = nullptr;
    if (!ev) return BSG_OK;
    if (!ev->ran) HIP_TRY(hipMalloc(&ev->ran, bsg::kGatherRanBytes));
    HIP_TRY(hipMemsetAsync(ev->ran, 0, bsg::kGatherRanBytes, d.stream));
    *ran = ev->ran;
    return BSG_OK;
}

int32_t enqueue_terms(bsg_ctx *ctx, Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint32_t slot, EventTriple *ev)
{
    bsg::ProbeArgs a;
    uint32_t lds = 0;
    if (int32_t rc = make_probe_args(ctx, d, g, bd, B, slot, ev, a, lds)) return rc;
    // the group's records FIRST: a batch without a term launches no probe, but its evaluation (enqueue_eval, same slot) still reads a
    // device-memory table — left stale, a group beyond the kernel arguments evaluated into another group's offsets (a GPU memory
    // fault that tools/fuzz_probe.py reached after 2 100 seeds: an all-constant batch against 129+ arenas behind a larger batch)
    bsg::ArenaTable<bsg::kMaxGroupArenas> t;
    const bsg::ArenaRef *ext = nullptr;
    if (int32_t rc = group_table(d, g, t, &ext)) return rc;
    d.ext_of_slot[slot] = ext;
    if (B.n_kinds == 0) return BSG_OK;
    const dim3 wg(bsg::kProbeThreads);
    hipEvent_t e0 = ev ? ev->k1s : nullptr, e1 = ev ? ev->k1e : nullptr;
    // Gather or stream, for the whole launch (bsh::launch_gathers): where every referenced kind's terms x k word loads cost less than
    // its filters' bytes, one wave per block reads the words it tests straight from the arena (k_probe_gather: no LDS, same verdict
    // words, same event slots); anything else keeps the streaming kernels and their per-block fallback.
    bsh::GatherKind gk[3];
    const uint64_t group_blocks = gather_kinds(g, B, gk);
    if (ctx->gather_kernel && bsh::launch_gathers(gk, B.n_kinds, group_blocks, B.many_terms, ctx->gather_cost)) {
        const dim3 ggrid((g.max_blocks + bsg::kGatherBlocks - 1) / bsg::kGatherBlocks, B.n_kinds, a.n_arenas);
        const uint32_t pad = gather_pad(ctx);
        uint64_t *ran = nullptr;
        if (int32_t rc = gather_counters(d, ev, &ran)) return rc;
        if (ext) hipExtLaunchKernelGGL(bsg::k_probe_gather_ext, ggrid, wg, pad, d.stream, e0, e1, 0, a, ext, ran);
        else     hipExtLaunchKernelGGL(bsg::k_probe_gather, ggrid, wg, pad, d.stream, e0, e1, 0, a, t, ran);
        HIP_TRY(hipGetLastError());
        ctx->last_probe_route.store(BSG_LAB_ROUTE_GATHER, std::memory_order_relaxed);
        if (ev) gathered_timing(*ev, B, gk, group_blocks);
        return BSG_OK;
    }
    const dim3 grid(g.max_blocks, B.n_kinds, a.n_arenas);
    ctx->last_probe_route.store(BSG_LAB_ROUTE_STREAM, std::memory_order_relaxed);
    if (ext && B.many_terms) hipExtLaunchKernelGGL(bsg::k_probe_terms_many_ext, grid, wg, lds, d.stream, e0, e1, 0, a, ext);
    else if (ext)            hipExtLaunchKernelGGL(bsg::k_probe_terms_ext, grid, wg, lds, d.stream, e0, e1, 0, a, ext);
    else if (B.many_terms)   hipExtLaunchKernelGGL(bsg::k_probe_terms_many, grid, wg, lds, d.stream, e0, e1, 0, a, t);
    else                     hipExtLaunchKernelGGL(bsg::k_probe_terms, grid, wg, lds, d.stream, e0, e1, 0, a, t);
    HIP_TRY(hipGetLastError());
    if (ev) ev->has_k1 = true;
    return BSG_OK;
}

// The doorbell behind whatever the stream holds so far: `seq` into page-locked memory, by a one-thread kernel (the runtime's stream
// memory operation, hipStreamWriteValue64, was measured in its place: no cheaper to enqueue, 2-3 us later to arrive).
int32_t ring_doorbell(Device &d, uint64_t *flag, uint64_t seq)
{
    hipLaunchKernelGGL(bsg::k_ring, dim3(1), dim3(1), 0, d.stream, flag, seq);
    HIP_TRY(hipGetLastError());
    return BSG_OK;
}

// A doorbell'd result on its way to the host: a page-locked buffer from the device's idle list, which k_probe_direct / k_query_direct
// write the survivors into, and the doorbell word behind the survivors.  The object lives OUTSIDE the scope of the device lock that
// take() is called under, because its destructor takes that lock: the buffer goes back to the device whatever way the call ends,
// behind a drain of the device's stream unless the call knows the kernels that write it to be over (drained).
struct DirectResult {
    Device *dev = nullptr;
    uint32_t di = 0;                 // the device's position in the context
    uint64_t *buf = nullptr;
    size_t cap = 0, bytes = 0;       // of the buffer; of the survivors in it
    uint64_t *flag = nullptr;
    uint64_t seq = 0;
    uint64_t *dst = nullptr;         // where the caller wants the survivors, if it copies them as they are
    bool drained = false;
    DirectResult() = default;
    DirectResult(DirectResult &&o) noexcept
        : dev(o.dev), di(o.di), buf(o.buf), cap(o.cap), bytes(o.bytes), flag(o.flag), seq(o.seq), dst(o.dst), drained(o.drained) { o.buf = nullptr; }
    DirectResult &operator=(DirectResult &&) = delete;
    ~DirectResult()
    {
        if (!buf) return;
        std::lock_guard<std::mutex> lk(dev->mu);
        if (!drained) (void)hipStreamSynchronize(dev->stream);
        dev->direct_bufs.emplace_back(buf, cap);
    }
    // under d.mu: a buffer for n_bytes of survivors, the device's workgroup counter, the bell armed with the device's next number
    int32_t take(Device &d, uint32_t device_index, size_t n_bytes)
    {
        dev = &d; di = device_index; bytes = n_bytes;
        const size_t need = n_bytes + 64;                  // the doorbell word sits behind the survivors
        for (size_t i = 0; i < d.direct_bufs.size(); ++i)
            if (d.direct_bufs[i].second >= need) { buf = d.direct_bufs[i].first; cap = d.direct_bufs[i].second; d.direct_bufs.erase(d.direct_bufs.begin() + i); break; }
        if (!buf) {
            uint64_t *p = nullptr;
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(64 * 1024, need), hipHostMallocDefault));
            buf = p; cap = std::max<size_t>(64 * 1024, need);
        }
        if (!d.d_direct_count) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_direct_count), 64));
            HIP_TRY(hipMemsetAsync(d.d_direct_count, 0, 64, d.stream));
        }
        flag = buf + (n_bytes + 7) / 8; seq = ++d.direct_seq;
        *reinterpret_cast<volatile uint64_t *>(flag) = 0;
        return BSG_OK;
    }
    // polls the bell for at most `limit`; false: it stayed silent (the caller asks the runtime)
    bool wait(std::chrono::microseconds limit) const
    {
        const auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq)
            if (std::chrono::steady_clock::now() - t0 > limit) return false;
        return true;
    }
};

// One dispatch for a small batch: bit tests + programs of every 64-block group (direct.hip.h); survivors to `out`.
// res: the doorbell'd buffer `out` belongs to (nullptr: survivors left on the device, no bell).
int32_t enqueue_direct(Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint64_t *out, const DirectResult *res, EventTriple *ev, uint32_t ring_wgs)
{
    bsg::DirectArgs a{};
    uint64_t *flag = res ? res->flag : nullptr;
    const uint64_t seq = d.direct_seq;                     // (== res->seq: taken under the same hold of the device lock)
    // (the kernel's own doorbell costs every workgroup a system-scope fence: beyond ring_wgs workgroups a dispatch behind it rings)
    const bool ring = flag && (uint64_t)g.max_G * g.shards.size() > ring_wgs;
    if (!ring) { a.done_count = d.d_direct_count; a.flag = flag; a.seq = seq; }
    a.th = bd.d_th; a.prog = bd.d_prog; a.chunk_len = bd.d_chunk_len; a.out = out;
    a.Tp = B.Tp; a.Wt = std::max(B.Wt, 1u); a.n_queries = B.n_queries; a.Lmax = B.Lmax; a.max_depth = B.max_depth; a.n_kinds = B.n_kinds;
    for (uint32_t y = 0; y < B.n_kinds; ++y) { a.kind[y] = B.kind[y]; a.term_begin[y] = B.term_begin[y]; a.term_count[y] = B.term_count[y]; }
    a.n_arenas = (uint32_t)g.shards.size();
    bsg::ArenaTable<bsg::kMaxGroupArenas> t;
    fill_refs(g, t.ar);
    hipExtLaunchKernelGGL(bsg::k_probe_direct, dim3(g.max_G, 1, a.n_arenas), dim3(bsg::kEvalThreads), bsg::direct_lds_bytes(a.Wt, B.max_depth),
                          d.stream, ev ? ev->k1s : nullptr, ev ? ev->k1e : nullptr, 0, a, t);
    HIP_TRY(hipGetLastError());
    if (ring) if (int32_t rc = ring_doorbell(d, flag, seq)) return rc;
    if (ev) {
        ev->has_k1 = true; ev->fused = true; ev->n_arenas = a.n_arenas;
        for (uint32_t y = 0; y < B.n_kinds; ++y)       // algorithmic bytes of the gather regime: k words of 8 bytes per (block, term)
            for (const ArenaShard *s : g.shards) ev->bytes += (uint64_t)s->n_blocks * B.term_count[y] * 10 * 8;
    }
    return BSG_OK;
}

// LDS of an evaluation workgroup (eval_block); sets the bit of a.identity_cw that selects eval_role_all:
// batches with the identity word list transpose a whole tile's words at once (eval_role_all) when that fits 64 KB of LDS
// Launches tiled by kEvalGroupTile (eval_tile_for: many groups) take row spans instead (eval_role_rows) where a span's transposed
// words and stacks, or its stage, fit lds_cap: `tile` becomes kEvalRowSpan and the bit that selects the body is set.  Deep programs
// and batches of many words keep eval_role_all.  lds_cap: 64 KB for the evaluation's own kernels; k_gather_fused passes what keeps
// three of its workgroups on a CU (the gather loses from two: profiles/probe_gather_lines_lab.txt §4).
uint32_t eval_lds_for(const Batch &B, bsg::EvalArgs &a, uint32_t &tile, uint32_t lds_cap = 64 * 1024)
{
    static const bool lab_serial = getenv("BSG_LAB_EVAL_SERIAL") != nullptr;   // lab only: the per-group walk for every batch
    static const char *lab_rows = getenv("BSG_LAB_EVAL_ROWS");                 // lab only: "0" = eval_role_all where the row spans would run
    if (B.identity_cw && !lab_serial && bsg::eval_lds_bytes(B.max_cw * bsg::kEvalGroupTile, B.max_depth * bsg::kEvalGroupTile) <= 64 * 1024) {
        a.identity_cw |= 2u;
        if (tile == bsg::kEvalGroupTile && !(lab_rows && atoi(lab_rows) == 0) && bsg::eval_rows_lds_bytes(B.max_cw, B.max_depth) <= lds_cap) {
            a.identity_cw |= 4u;
            tile = bsg::kEvalRowSpan;
            return bsg::eval_rows_lds_bytes(B.max_cw, B.max_depth);
        }
        return bsg::eval_lds_bytes(B.max_cw * bsg::kEvalGroupTile, B.max_depth * bsg::kEvalGroupTile);
    }
    return bsg::eval_lds_bytes(B.max_cw, B.max_depth);
}

// K2: programs over V[slot] -> out[slot].
// out_override: the survivors go there (device-visible memory in the group's layout) instead of out[slot].
// ext_at: g is a CHUNK of the group in the slot (pipeline_chunked) and its records start there, inside the group's device table.
int32_t enqueue_eval(Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint32_t slot, EventTriple *ev, uint64_t *out_override = nullptr,
                     hipStream_t on = nullptr, const bsg::ArenaRef *ext_at = nullptr)
{
    bsg::EvalArgs a;
    if (int32_t rc = make_eval_args(d, g, bd, B, slot, a)) return rc;
    if (out_override) a.out = out_override;
    const hipStream_t stream = on ? on : d.stream;
    uint32_t tile = eval_tile_for(g);
    bsg::ArenaTable<bsg::kMaxGroupArenas> t;
    const bsg::ArenaRef *ext = nullptr;
    if (ext_at) ext = ext_at;
    else if (g.shards.size() <= bsg::kMaxGroupArenas) fill_refs(g, t.ar);
    else ext = d.ext_of_slot[slot];         // written (or found in the device's table cache) by this group's probe dispatch (enqueue_terms), same slot, same stream
    const uint32_t lds = eval_lds_for(B, a, tile);        // (row spans: tile becomes the span)
    const uint32_t nx = (g.max_G + tile - 1) / tile;
    const uint64_t n_wg = (uint64_t)(B.n_chunks * (uint64_t)a.n_arenas + 7) / 8 * 8 * nx;
    if (n_wg > 0x7FFFFFFFull) return fail(BSG_E_UNSUPPORTED, "evaluation launch of %llu workgroups", (unsigned long long)n_wg);
    if (ext) hipExtLaunchKernelGGL(bsg::k_eval_programs_ext, dim3((uint32_t)n_wg), dim3(bsg::kEvalThreads), lds, stream, ev ? ev->k2s : nullptr,
                                   ev ? ev->k2e : nullptr, 0, a, ext, tile, nx, B.n_chunks);
    else hipExtLaunchKernelGGL(bsg::k_eval_programs, dim3((uint32_t)n_wg), dim3(bsg::kEvalThreads), lds, stream, ev ? ev->k2s : nullptr,
                               ev ? ev->k2e : nullptr, 0, a, t, tile, nx, B.n_chunks);
    HIP_TRY(hipGetLastError());
    if (ev) ev->has_k2 = true;
    return BSG_OK;
}

// One launch per group, evaluation folded in per tile of 64 x tile_groups blocks (k_probe_eval): verdicts into V[slot],
// survivors into out[slot] by the last arrivals of every tile.
bool fold_applies(const bsg_ctx *ctx, const Batch &B, uint32_t flags)
{
    return ctx->fold_helpers > 0 && !(flags & BSG_PROBE_NOFUSE) && !B.many_terms && B.n_kinds > 0 && B.identity_cw && B.max_cw == std::max(B.Wt, 1u) &&
           bsg::fold_eval_lds_bytes(bsg::kFoldGroupTile, B.max_cw, B.max_depth) <= 64 * 1024;
}

int32_t enqueue_fold(bsg_ctx *ctx, Device &d, const Group &g, const BatchDev &bd, const Batch &B, uint32_t slot, EventTriple *ev)
{
    bsg::FoldArgs f{};
    uint32_t lds = 0;
    if (int32_t rc = make_probe_args(ctx, d, g, bd, B, slot, ev, f.p, lds)) return rc;
    if (int32_t rc = make_eval_args(d, g, bd, B, slot, f.e)) return rc;
    // verdict entries are 16 bytes here (word + tag): twice the words of the plain layout, zeroed when (re)allocated so that no
    // entry can carry a tag by accident
    const uint64_t v_need = 2 * std::max<uint64_t>(g.v_words, 1);
    if (v_need > d.V[slot].cap) {
        HIP_TRY(hipStreamSynchronize(d.stream));
        HIP_TRY(d.V[slot].reserve(v_need));
        HIP_TRY(hipMemsetAsync(d.V[slot].p, 0, d.V[slot].cap * sizeof(uint64_t), d.stream));
    }
    f.p.V = d.V[slot].p;
    f.e.V = d.V[slot].p;
    f.p.seq = ++d.fold_seq;
    f.tile_groups = eval_tile_for(g) > 1 ? bsg::kFoldGroupTile : 1u;
    f.helpers = ctx->fold_helpers;
    static const bool lab_skip = getenv("BSG_LAB_FOLD_SKIP") != nullptr;   // lab only: nobody evaluates (what the probe side of the fold costs by itself)
    if (lab_skip) f.helpers = 0;
    static const uint32_t lab_fold = getenv("BSG_LAB_FOLD") ? (uint32_t)atoi(getenv("BSG_LAB_FOLD")) : 0u;
    f.lab = lab_fold;
    f.n_kinds = B.n_kinds;
    lds = std::max(lds, bsg::fold_eval_lds_bytes(f.tile_groups, B.max_cw, B.max_depth));
    bsg::ArenaTable<bsg::kMaxGroupArenas> t;
    fill_refs(g, t.ar);
    hipExtLaunchKernelGGL(bsg::k_probe_eval, dim3(g.max_blocks, B.n_kinds, f.p.n_arenas), dim3(bsg::kProbeThreads), lds, d.stream,
                          ev ? ev->k1s : nullptr, ev ? ev->k1e : nullptr, 0, f, t);
    HIP_TRY(hipGetLastError());
    if (ev) { ev->has_k1 = true; ev->folded = true; }
    return BSG_OK;
}

// One launch: K1 of the current group (slot) + K2 of the previous group (pslot).  See k_probe_fused.
int32_t enqueue_fused(bsg_ctx *ctx, Device &d, const Group &g, uint32_t slot, const Group &pg, uint32_t pslot, const BatchDev &bd,
                      const Batch &B, EventTriple *ev)
{
    bsg::FusedArgs f{};
    uint32_t lds = 0;
    if (int32_t rc = make_probe_args(ctx, d, g, bd, B, slot, ev, f.p, lds)) return rc;
    if (int32_t rc = make_eval_args(d, pg, bd, B, pslot, f.e)) return rc;
    f.n_kinds = B.n_kinds;
    f.n_probe = g.max_blocks * B.n_kinds * f.p.n_arenas;
    f.eval_pairs = (B.n_chunks + 1) / 2;
    f.eval_lds_half = bsg::eval_lds_bytes(B.max_cw, B.max_depth);
    lds = std::max(lds, 2 * f.eval_lds_half);
    f.eval_tile = eval_tile_for(pg);
    const uint64_t grid = (uint64_t)f.n_probe + (uint64_t)(pg.max_G + f.eval_tile - 1) / f.eval_tile * f.eval_pairs * f.e.n_arenas;
    if (grid > 0x7FFFFFFFull) return fail(BSG_E_UNSUPPORTED, "fused launch of %llu workgroups", (unsigned long long)grid);
    bsg::ArenaTable<bsg::kMaxFusedArenas> tp, te;              // (the caller keeps fused groups within kMaxFusedArenas)
    fill_refs(g, tp.ar);
    fill_refs(pg, te.ar);
    hipExtLaunchKernelGGL(bsg::k_probe_fused, dim3((uint32_t)grid), dim3(bsg::kProbeThreads), lds, d.stream, ev ? ev->k1s : nullptr,
                          ev ? ev->k1e : nullptr, 0, f, tp, te);
    HIP_TRY(hipGetLastError());
    if (ev) { ev->has_k1 = true; ev->fused = true; }
    return BSG_OK;
}

// One launch of a group probed in chunks: the gather of chunk `gc` (its records from ext + a0) + the evaluation of the chunk before
// it, `ec` (from ext + e0), both in the group's scratch slot.  See k_gather_fused.  tile: eval_tile_for the whole group.
int32_t enqueue_gather_fused(bsg_ctx *ctx, Device &d, const Group &gc, uint32_t a0, const Group &ec, uint32_t e0, const bsg::ArenaRef *ext,
                             uint32_t tile, bool spread, const BatchDev &bd, const Batch &B, uint32_t slot, EventTriple *ev)
{
    bsg::GatherFusedArgs f{};
    uint32_t lds = 0;
    if (int32_t rc = make_probe_args(ctx, d, gc, bd, B, slot, ev, f.p, lds)) return rc;
    if (int32_t rc = make_eval_args(d, ec, bd, B, slot, f.e)) return rc;
    // (the pad is per workgroup, so it caps the evaluation workgroups of this dispatch too; row spans only where three workgroups keep a CU)
    lds = std::max(eval_lds_for(B, f.e, tile, bsh::gather_lds_pad(3)), gather_pad(ctx));
    f.a0 = a0; f.e0 = e0;
    f.spread = spread ? 1u : 0u;
    f.n_kinds = B.n_kinds;
    f.n_chunks = B.n_chunks;
    f.gather_nx = (gc.max_blocks + bsg::kGatherBlocks - 1) / bsg::kGatherBlocks;
    f.eval_tile = tile;
    f.eval_nx = (ec.max_G + tile - 1) / tile;
    const uint64_t n_eval = (uint64_t)(B.n_chunks * (uint64_t)f.e.n_arenas + 7) / 8 * 8 * f.eval_nx;
    const uint64_t octets = n_eval / 8 + ((uint64_t)f.gather_nx * B.n_kinds * f.p.n_arenas + 7) / 8;
    if (octets * 8 > 0x7FFFFFFFull) return fail(BSG_E_UNSUPPORTED, "chunked gather launch of %llu workgroups", (unsigned long long)(octets * 8));
    f.n_eval = (uint32_t)n_eval;
    f.n_octets = (uint32_t)octets;
    uint64_t *ran = nullptr;
    if (int32_t rc = gather_counters(d, ev, &ran)) return rc;
    hipExtLaunchKernelGGL(bsg::k_gather_fused, dim3((uint32_t)(octets * 8)), dim3(bsg::kProbeThreads), lds, d.stream, ev ? ev->k1s : nullptr,
                          ev ? ev->k1e : nullptr, 0, f, ext, ran);
    HIP_TRY(hipGetLastError());
    if (ev) {
        bsh::GatherKind gk[3];
        const uint64_t blocks = gather_kinds(gc, B, gk);
        gathered_timing(*ev, B, gk, blocks);
        ev->fused = true;
    }
    return BSG_OK;
}

// Probes batch B against every arena of the list.  Per device the launches are software-pipelined on one in-order stream
//   K1(g0) | F(g1) = K1(g1) + K2(g0) | F(g2) = K1(g2) + K2(g1) | ... | K2(g_last)
// where a group g_i is up to ctx->group_limit arenas probed by ONE dispatch and F = k_probe_fused: the program evaluation
// of group i-1 rides in the grid that streams group i's bitsets.  V/out are double-buffered by group parity.  Survivors
// leave through the device's copy stream (D2H of group i overlaps the kernels of group i+1); contexts on several devices
// enqueue on all of them before waiting on any, then interleave the shards' bitsets on the host.
// out_dev != nullptr (single-device contexts): survivors are left at that device pointer instead, in the same layout.
// (Measured on MI355X in round 1: per-arena cross-stream events cost the host 3-4 us each — per group they are noise.)
int32_t probe_arenas(bsg_ctx *ctx, const std::vector<std::shared_ptr<Arena>> &arenas, const Batch &B, uint32_t flags,
                     uint64_t *out_survivors, uint64_t *out_dev, uint32_t *rows_hdr = nullptr);

// A COMPOSITE batch (one beyond a launch's limits, cut into runs of queries by bsg_batch_create): every run probes on its own;
// its rows are scattered into the caller's layout (arena i: [n_queries][G_i], the run's rows [q0, q0 + nq) of it) on the host.
int32_t probe_composite(bsg_ctx *ctx, const std::vector<std::shared_ptr<Arena>> &arenas, const Batch &B, uint32_t flags,
                        uint64_t *out_survivors, uint64_t *out_dev)
{
    const uint32_t n_arenas = (uint32_t)arenas.size();
    if (out_dev) return fail(BSG_E_UNSUPPORTED, "a batch beyond one launch's limits cannot leave its survivors at a device pointer");
    if (!out_survivors) {
        for (auto &sub : B.subs) if (int32_t rc = probe_arenas(ctx, arenas, *sub, flags, nullptr, nullptr)) return rc;
        return BSG_OK;
    }
    if (flags & BSG_PROBE_ASYNC) return fail(BSG_E_UNSUPPORTED, "a batch beyond one launch's limits needs a synchronous probe");
    const std::vector<uint64_t> aoff = bsh::survivor_offsets(n_arenas, B.n_queries, ArenaBlocks{arenas});
    std::vector<uint64_t> tmp;
    for (size_t si = 0; si < B.subs.size(); ++si) {
        const Batch &S = *B.subs[si];
        tmp.assign(std::max<uint64_t>(1, (uint64_t)S.n_queries * (aoff[n_arenas] / std::max(B.n_queries, 1u))), 0);
        if (int32_t rc = probe_arenas(ctx, arenas, S, flags, tmp.data(), nullptr)) return rc;
        uint64_t o = 0;
        for (uint32_t i = 0; i < n_arenas; ++i) {
            const uint64_t G = bsh::words64(arenas[i]->n_blocks);
            memcpy(out_survivors + aoff[i] + (uint64_t)B.sub_q0[si] * G, tmp.data() + o, (uint64_t)S.n_queries * G * 8);
            o += (uint64_t)S.n_queries * G;
        }
    }
    return BSG_OK;
}

// The layout of survivor rows (host/probe_plan.hpp) for these arenas on a context of nd devices.
using bsh::RowsLayout;

RowsLayout rows_layout(const std::vector<std::shared_ptr<Arena>> &arenas, uint32_t nd, uint32_t n_queries)
{
    return bsh::rows_layout(nd, (uint32_t)arenas.size(), n_queries, [&arenas](uint32_t d, uint32_t i) { return arenas[i]->shards[d].n_blocks; });
}

// the device pointers behind the caller's page-locked row slots and headers (per device); every check first, then the headers of
// shards without blocks (no launch ever touches them) are set to NONE
int32_t rows_targets(bsg_ctx *ctx, const std::vector<std::shared_ptr<Arena>> &arenas, const Batch &B, uint64_t *out_survivors, uint64_t *out_dev,
                     uint32_t *rows_hdr, std::vector<uint64_t *> &d_rows, std::vector<uint32_t *> &d_hdr, bool packed)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    if (!B.subs.empty() || !out_survivors || out_dev)
        return fail(BSG_E_UNSUPPORTED, "survivor rows need a batch within one launch's limits and host buffers");
    d_rows.assign(nd, nullptr); d_hdr.assign(nd, nullptr);
    for (uint32_t di = 0; di < nd; ++di) {
        std::lock_guard<std::mutex> lk(ctx->devs[di]->mu);
        if (int32_t rc = use_device(*ctx->devs[di])) return rc;
        if (hipHostGetDevicePointer(reinterpret_cast<void **>(&d_rows[di]), out_survivors, 0) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void **>(&d_hdr[di]), rows_hdr, 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BSG_E_INVALID, "survivor rows are written by the device: out_rows and out_hdr must be page-locked memory (bsg_pinned_alloc / bsg_host_register)");
        }
    }
    for (uint32_t di = 0; di < nd; ++di)
        for (size_t i = 0; i < arenas.size(); ++i)
            if (arenas[i]->shards[di].n_blocks == 0) {
                const size_t at = ((size_t)di * arenas.size() + i) * B.n_queries;          // (packed: one byte per header, same index)
                if (packed) memset(reinterpret_cast<uint8_t *>(rows_hdr) + at, 0, B.n_queries);
                else memset(rows_hdr + at, 0, (size_t)B.n_queries * 4);
            }
    return BSG_OK;
}

// One probe_arenas call: its arguments, what is decided once for all devices, and what the devices leave for the wait and the merge.
struct ProbeCall {
    bsg_ctx *ctx;
    const std::vector<std::shared_ptr<Arena>> &arenas;
    const Batch &B;
    uint32_t flags;
    uint64_t *out_survivors, *out_dev;
    uint32_t *rows_hdr;            // != nullptr (bsg_probe_many_rows): out_survivors and rows_hdr are page-locked, written by the device
    uint32_t nd, n_arenas;
    bool timed, fuse, packed;
    uint32_t fuse_max_arenas, limit;
    std::vector<uint64_t> out_off;                 // arena i's survivors start at out_survivors + out_off[i]
    RowsLayout RL;
    std::vector<uint64_t *> d_rows;
    std::vector<uint32_t *> d_hdr;
    std::vector<std::vector<uint64_t>> parts;      // several devices, host output: every device's shard bitsets land in a buffer of its own
    std::vector<DirectResult> direct;              // k_probe_direct results waiting in page-locked buffers for the stream to drain
};

// the ways a group's survivors leave out[slot] once its evaluation is enqueued
enum class SurvivorsOut { kStay, kRows, kInlineCopy, kCopyStream };

// One device's part of a probe_arenas call, under the device's lock: its groups, where their survivors go and how, and the two
// points of bookkeeping around every evaluation.
struct DeviceRun {
    ProbeCall &c;
    Device &d;
    const BatchDev &bd;
    uint32_t di;
    std::vector<Group> groups;
    std::vector<uint64_t> goff;          // where each group's survivors go (u64 offset from host_base / out_dev)
    uint64_t *host_base = nullptr;
    SurvivorsOut way = SurvivorsOut::kStay;
    std::vector<EventTriple> evs;        // per group; tflag: the group is timed
    std::vector<uint8_t> tflag;

    EventTriple *ev(size_t gi) { return tflag[gi] ? &evs[gi] : nullptr; }
    bool fusable(size_t gi) const        // groups gi - 1 and gi in one k_probe_fused launch
    {
        return c.fuse && groups[gi].shards.size() <= c.fuse_max_arenas && groups[gi - 1].shards.size() <= c.fuse_max_arenas;
    }
    int32_t plan();
    bool direct_applies() const;
    int32_t direct();
    int32_t pipeline();
    int32_t pipeline_chunked(const std::vector<uint32_t> &sizes);
    int32_t before_eval(uint32_t slot);
    int32_t after_eval(size_t gi, uint32_t slot);
    int32_t rows_out(size_t gi, uint32_t slot);
    int32_t inline_copy_out(size_t gi, uint32_t slot);
    int32_t copy_stream_out(size_t gi, uint32_t slot);
};

// The groups of this device (host/probe_plan.hpp), their output offsets and the way out of their survivors.
// (measured, round 5: a run of 129 .. 256 arenas as TWO kernel-argument groups instead of one group behind two
// k_write_arena_table dispatches loses — 200 shards of 125 blocks: probe 2 x 74.4 vs 139.4 us, evaluation 2 x 11.3 vs 18.3 us,
// 10.11 vs 9.62 us per step — the second ramp costs more than the two table writes: profiles/r05_step.txt)
int32_t DeviceRun::plan()
{
    groups = bsh::plan_groups<Group>(c.n_arenas, ShardBlocks{c.arenas, di}, c.B.n_queries, c.B.Wt, c.limit);
    for (Group &g : groups) {
        g.shards.reserve(g.index.size());
        for (uint32_t i : g.index) g.shards.push_back(&c.arenas[i]->shards[di]);
    }
    if (groups.empty()) return BSG_OK;
    if (!c.parts.empty()) {
        goff = bsh::group_offsets(groups, nullptr);
        c.parts[di].resize(goff.back());
        host_base = c.parts[di].data();
    } else {
        goff = bsh::group_offsets(groups, c.out_off.data());
        host_base = c.out_survivors;
    }
    // latency path (a single interactive query): one group, a small synchronous result — the copy rides the compute
    // stream, no cross-stream events
    if (c.rows_hdr) way = SurvivorsOut::kRows;
    else if (!c.out_survivors && !c.out_dev) way = SurvivorsOut::kStay;
    else if (groups.size() == 1 && !(c.flags & BSG_PROBE_ASYNC) && groups[0].out_words * 8 <= (1u << 20)) way = SurvivorsOut::kInlineCopy;
    else way = SurvivorsOut::kCopyStream;
    if (way == SurvivorsOut::kCopyStream) HIP_TRY(ensure_copy_stream(d));
    return BSG_OK;
}

// one interactive query (a small synchronous batch with a few terms against one group): one dispatch, and the
// survivors are written straight into page-locked host memory — one launch and one wait instead of three enqueues
bool DeviceRun::direct_applies() const
{
    const Batch &B = c.B;
    uint32_t real_terms = 0;
    for (uint32_t y = 0; y < B.n_kinds; ++y) real_terms += B.term_count[y];
    return way == SurvivorsOut::kInlineCopy && !(c.flags & BSG_PROBE_NOFUSE) && B.n_chunks == 1 && B.identity_cw && !B.many_terms &&
           groups[0].shards.size() <= bsg::kMaxGroupArenas && real_terms <= c.ctx->direct_max_terms &&
           bsg::direct_lds_bytes(std::max(B.Wt, 1u), B.max_depth) <= 64 * 1024;
}

int32_t DeviceRun::direct()
{
    EventTriple ev0;
    if (c.timed) if (int32_t rc = take_events(c.ctx, d, ev0)) return rc;
    uint64_t *target = c.out_dev ? c.out_dev + goff[0] : nullptr;
    const DirectResult *res = nullptr;
    if (!c.out_dev) {
        c.direct.emplace_back();
        if (int32_t rc = c.direct.back().take(d, di, groups[0].out_words * 8)) return rc;
        c.direct.back().dst = host_base + goff[0];
        res = &c.direct.back();
        target = res->buf;
    }
    if (int32_t rc = enqueue_direct(d, groups[0], bd, c.B, target, res, c.timed ? &ev0 : nullptr, c.ctx->solo_ring_wgs)) return rc;
    if (c.timed) d.pending.push_back(ev0);
    return BSG_OK;
}

// out[slot] is about to be overwritten
int32_t DeviceRun::before_eval(uint32_t slot)
{
    if (d.copy_busy[slot]) { HIP_TRY(hipStreamWaitEvent(d.stream, d.ev_copy[slot], 0)); d.copy_busy[slot] = false; }
    return BSG_OK;
}

// K2 of group gi is enqueued: its timing triple is complete, its survivors leave
int32_t DeviceRun::after_eval(size_t gi, uint32_t slot)
{
    if (tflag[gi]) d.pending.push_back(evs[gi]);
    switch (way) {
    case SurvivorsOut::kRows: return rows_out(gi, slot);
    case SurvivorsOut::kInlineCopy: return inline_copy_out(gi, slot);
    case SurvivorsOut::kCopyStream: return copy_stream_out(gi, slot);
    case SurvivorsOut::kStay: break;
    }
    return BSG_OK;
}

// the group's rows, tagged and compacted, straight into the caller's page-locked buffers (same stream: ordered
// behind the evaluation and ahead of the next use of out[slot])
int32_t DeviceRun::rows_out(size_t gi, uint32_t slot)
{
    const Group &g = groups[gi];
    const uint32_t Q = c.B.n_queries;
    // (packed rows: byte headers — the device's slice starts at BYTE di * n_arenas * n_queries of the header buffer)
    uint32_t *hdr_base = c.packed ? reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(c.d_hdr[di]) + (size_t)di * c.n_arenas * Q)
                                  : c.d_hdr[di] + (size_t)di * c.n_arenas * Q;
    bsg::RowsArgs ra{d.out[slot].p, c.d_rows[di] + c.RL.row_base[di], hdr_base, Q};
    for (size_t i0 = 0; i0 < g.shards.size(); i0 += bsg::kMaxRowsArenas) {      // (two tables ride in the kernel arguments: runs of 64 arenas)
        const size_t n = std::min<size_t>(bsg::kMaxRowsArenas, g.shards.size() - i0);
        bsg::ArenaTable<bsg::kMaxRowsArenas> t;
        bsg::RowsTable<bsg::kMaxRowsArenas> dst;
        fill_refs(g, t.ar, i0, n);
        for (size_t i = 0; i < n; ++i) dst.d[i] = bsg::RowsDst{c.RL.arena_off[di][g.index[i0 + i]], (uint64_t)g.index[i0 + i] * Q};
        if (c.packed) hipLaunchKernelGGL(bsg::k_survivor_rows_packed, dim3((Q + 255) / 256, (uint32_t)n), dim3(256), 0, d.stream, ra, t, dst);
        else hipLaunchKernelGGL(bsg::k_survivor_rows, dim3((Q + 255) / 256, (uint32_t)n), dim3(256), 0, d.stream, ra, t, dst);
        HIP_TRY(hipGetLastError());
    }
    return BSG_OK;
}

int32_t DeviceRun::inline_copy_out(size_t gi, uint32_t slot)
{
    HIP_TRY(hipMemcpyAsync(c.out_dev ? (void *)(c.out_dev + goff[gi]) : (void *)(host_base + goff[gi]), d.out[slot].p, groups[gi].out_words * 8,
                           c.out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, d.stream));
    return BSG_OK;
}

int32_t DeviceRun::copy_stream_out(size_t gi, uint32_t slot)
{
    const uint64_t bytes = groups[gi].out_words * 8;
    HIP_TRY(hipEventRecord(d.ev_eval[slot], d.stream));
    HIP_TRY(hipStreamWaitEvent(d.copy_stream, d.ev_eval[slot], 0));
    if (c.out_dev) HIP_TRY(hipMemcpyAsync(c.out_dev + goff[gi], d.out[slot].p, bytes, hipMemcpyDeviceToDevice, d.copy_stream));
    else HIP_TRY(hipMemcpyAsync(host_base + goff[gi], d.out[slot].p, bytes, hipMemcpyDeviceToHost, d.copy_stream));
    HIP_TRY(hipEventRecord(d.ev_copy[slot], d.copy_stream));
    d.copy_busy[slot] = true;
    return BSG_OK;
}

// ONE group probed in chunks of consecutive arenas (bsh::pipeline_chunks), all in scratch slot 0:
//   k_probe_gather_ext(chunk 0) | k_gather_fused(gather chunk i, evaluate chunk i - 1) ... | k_eval_programs_ext(last chunk)
// The group's records lie in its device-memory table whatever its size, and every arena keeps the v_off / out_off it has in the
// whole group: the chunks fill the slot's V and out side by side, and the survivors leave once, behind the last evaluation.
// Timing: one triple per chunk — chunk 0's gather a terms kernel, every k_gather_fused a fused dispatch that counts the arenas it
// gathers, the last evaluation the eval kernel of the last triple: every arena is counted once.
int32_t DeviceRun::pipeline_chunked(const std::vector<uint32_t> &sizes)
{
    bsg_ctx *ctx = c.ctx;
    const Batch &B = c.B;
    const Group &g = groups[0];
    const size_t nc = sizes.size();
    std::vector<Group> chunks(nc);
    std::vector<uint32_t> first(nc + 1, 0);
    for (size_t ci = 0, i = 0; ci < nc; ++ci) {
        first[ci + 1] = first[ci] + sizes[ci];
        for (; i < first[ci + 1]; ++i) group_add(chunks[ci], B.n_queries, B.Wt, *g.shards[i], g.index[i]);
    }
    evs.resize(1);
    tflag.assign(1, 0);                            // (after_eval pushes no triple of its own: the chunks' triples go below)
    const bool timed = c.timed && (ctx->timed_stride <= 1 || (ctx->timed_counter++ % ctx->timed_stride) == ctx->timed_stride / 2);
    std::vector<EventTriple> cev(timed ? nc : 0);
    for (EventTriple &e : cev) if (int32_t rc = take_events(ctx, d, e)) return rc;
    auto cv = [&](size_t ci) { return timed ? &cev[ci] : nullptr; };
    // the whole group's scratch and records first: the chunks' own requests below then find both in place
    HIP_TRY(d.V[0].reserve(std::max<uint64_t>(g.v_words, 1)));
    HIP_TRY(d.out[0].reserve(std::max<uint64_t>(g.out_words, 1)));
    bsg::ArenaTable<bsg::kMaxGroupArenas> t;
    const bsg::ArenaRef *ext = nullptr;
    if (int32_t rc = group_table(d, g, t, &ext, true)) return rc;
    d.ext_of_slot[0] = ext;
    const uint32_t tile = eval_tile_for(g);
    const uint32_t place = (uint32_t)(ctx->pipeline_key >> 24) & 3u;      // 0: the default, 1: evaluation octets in front, 2: spread
    const bool spread = place ? place == 2u : bsh::kPipelineSpread;
    {
        bsg::ProbeArgs a;
        uint32_t lds = 0;
        if (int32_t rc = make_probe_args(ctx, d, chunks[0], bd, B, 0, cv(0), a, lds)) return rc;
        const dim3 ggrid((chunks[0].max_blocks + bsg::kGatherBlocks - 1) / bsg::kGatherBlocks, B.n_kinds, a.n_arenas);
        uint64_t *ran = nullptr;
        if (int32_t rc = gather_counters(d, cv(0), &ran)) return rc;
        hipExtLaunchKernelGGL(bsg::k_probe_gather_ext, ggrid, dim3(bsg::kProbeThreads), gather_pad(ctx), d.stream, timed ? cev[0].k1s : nullptr,
                              timed ? cev[0].k1e : nullptr, 0, a, ext, ran);
        HIP_TRY(hipGetLastError());
        if (timed) {
            bsh::GatherKind gk[3];
            const uint64_t blocks = gather_kinds(chunks[0], B, gk);
            gathered_timing(cev[0], B, gk, blocks);
        }
    }
    if (int32_t rc = before_eval(0)) return rc;
    for (size_t ci = 1; ci < nc; ++ci)
        if (int32_t rc = enqueue_gather_fused(ctx, d, chunks[ci], first[ci], chunks[ci - 1], first[ci - 1], ext, tile, spread, bd, B, 0, cv(ci))) return rc;
    if (int32_t rc = enqueue_eval(d, chunks[nc - 1], bd, B, 0, cv(nc - 1), nullptr, nullptr, ext + first[nc - 1])) return rc;
    ctx->last_probe_route.store(BSG_LAB_ROUTE_GATHER_CHUNKED, std::memory_order_relaxed);
    for (EventTriple &e : cev) d.pending.push_back(e);
    return after_eval(0, 0);
}

// The software pipeline over the groups; per group one of four arms: folded (one dispatch per group), fused with the evaluation of
// the group before, or the two kernels — the evaluation of the group before on the device's stream, or (tail split) on a second one.
int32_t DeviceRun::pipeline()
{
    bsg_ctx *ctx = c.ctx;
    const Batch &B = c.B;
    bool fold = fold_applies(ctx, B, c.flags);
    for (const Group &g : groups) fold = fold && g.shards.size() <= bsg::kMaxGroupArenas;     // (k_probe_eval keeps its records in the kernel arguments)
    // A short run — ONE group, survivors left on the device — ends in a serial tail: the whole group's program evaluation behind
    // its stream (11 of 132 us at 20 arenas of C2).  tail_split (bsg_set_lab key 19, percent) cuts the group in two dispatches'
    // worth: the first part's evaluation runs on a second stream while the second part streams, and only the second part's
    // evaluation is left behind the stream.  Two groups that fuse are left to the fused launch.
    // a single group that gathers may run in chunks, its evaluation under its own gather (bsh::pipeline_chunks decides: first by
    // everything that costs nothing to know, and only a run it would chunk is asked whether its launch gathers)
    if (groups.size() == 1 && ctx->pipeline_key != 1 && groups[0].shards.size() >= 2) {
        const Group &g = groups[0];
        uint64_t g_blocks = 0;
        for (const ArenaShard *s : g.shards) g_blocks += s->n_blocks;
        bsh::PipelineCase pc{true, !B.many_terms && B.identity_cw && B.n_kinds > 0, (uint32_t)groups.size(),
                             ctx->fold_helpers > 0 || ctx->tail_split_pct > 0 || (c.flags & BSG_PROBE_NOFUSE) != 0};
        if (bsh::pipeline_chunks((uint32_t)g.shards.size(), g_blocks, pc, ctx->pipeline_key).size() > 1) {
            pc.gathers = group_gathers(ctx, g, B);
            const std::vector<uint32_t> sizes = bsh::pipeline_chunks((uint32_t)g.shards.size(), g_blocks, pc, ctx->pipeline_key);
            if (sizes.size() > 1) return pipeline_chunked(sizes);
        }
    }
    const bool tail_mode = ctx->tail_split_pct && way == SurvivorsOut::kStay && !fold;
    if (tail_mode && groups.size() == 1)
        if (const size_t n0 = bsh::tail_split_cut(groups[0].shards.size(), ctx->tail_split_pct, bsg::kMaxGroupArenas)) {
            const Group whole = std::move(groups[0]);
            groups.assign(2, Group{});
            for (size_t i = 0; i < whole.shards.size(); ++i) group_add(groups[i < n0 ? 0 : 1], B.n_queries, B.Wt, *whole.shards[i], whole.index[i]);
            goff.assign(3, 0);
        }
    const bool split = tail_mode && groups.size() == 2 && !fusable(1);
    if (split && !d.aux_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&d.aux_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&d.ev_aux[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&d.ev_aux[1], hipEventDisableTiming));
    }
    evs.resize(groups.size());
    tflag.assign(groups.size(), 0);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const uint32_t slot = (uint32_t)(gi & 1);
        tflag[gi] = c.timed && (ctx->timed_stride <= 1 || (ctx->timed_counter++ % ctx->timed_stride) == ctx->timed_stride / 2);
        if (tflag[gi]) if (int32_t rc = take_events(ctx, d, evs[gi])) return rc;
        if (fold) {
            // one dispatch per group: the survivors of group gi are complete when its kernel is
            if (int32_t rc = before_eval(slot)) return rc;
            if (int32_t rc = enqueue_fold(ctx, d, groups[gi], bd, B, slot, ev(gi))) return rc;
            if (int32_t rc = after_eval(gi, slot)) return rc;
        } else if (gi > 0 && fusable(gi)) {
            // a fused launch's own timestamps cover the streaming of group gi AND the evaluation of group gi-1
            if (int32_t rc = before_eval(slot ^ 1)) return rc;
            if (int32_t rc = enqueue_fused(ctx, d, groups[gi], slot, groups[gi - 1], slot ^ 1, bd, B, ev(gi))) return rc;
            if (int32_t rc = after_eval(gi - 1, slot ^ 1)) return rc;
        } else if (gi > 0 && split) {
            // the evaluation of the first part: on the second stream, behind the first part's probe, beside the second part's
            if (int32_t rc = before_eval(slot ^ 1)) return rc;
            HIP_TRY(hipEventRecord(d.ev_aux[0], d.stream));
            HIP_TRY(hipStreamWaitEvent(d.aux_stream, d.ev_aux[0], 0));
            if (int32_t rc = enqueue_eval(d, groups[gi - 1], bd, B, slot ^ 1, ev(gi - 1), nullptr, d.aux_stream)) return rc;
            HIP_TRY(hipEventRecord(d.ev_aux[1], d.aux_stream));
            if (int32_t rc = after_eval(gi - 1, slot ^ 1)) return rc;
            if (int32_t rc = enqueue_terms(ctx, d, groups[gi], bd, B, slot, ev(gi))) return rc;
            HIP_TRY(hipStreamWaitEvent(d.stream, d.ev_aux[1], 0));      // the stream's end is the call's end: it joins the second stream
        } else {
            if (gi > 0) {
                if (int32_t rc = before_eval(slot ^ 1)) return rc;
                if (int32_t rc = enqueue_eval(d, groups[gi - 1], bd, B, slot ^ 1, ev(gi - 1))) return rc;
                if (int32_t rc = after_eval(gi - 1, slot ^ 1)) return rc;
            }
            if (int32_t rc = enqueue_terms(ctx, d, groups[gi], bd, B, slot, ev(gi))) return rc;
        }
    }
    if (!fold) {
        const size_t gl = groups.size() - 1;
        const uint32_t slot = (uint32_t)(gl & 1);
        if (int32_t rc = before_eval(slot)) return rc;
        if (int32_t rc = enqueue_eval(d, groups[gl], bd, B, slot, ev(gl))) return rc;
        if (int32_t rc = after_eval(gl, slot)) return rc;
    }
    return BSG_OK;
}

// everything device di owes the call, enqueued under its lock
int32_t enqueue_device(ProbeCall &c, uint32_t di)
{
    Device &d = *c.ctx->devs[di];
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    DeviceRun r{c, d, c.B.dev[di], di};
    if (int32_t rc = r.plan()) return rc;
    if (r.groups.empty()) return BSG_OK;
    return r.direct_applies() ? r.direct() : r.pipeline();
}

// k_probe_direct rings a doorbell in page-locked memory when its last workgroup is done: reading our own memory is
// cheaper than asking the runtime.  Completion is tracked PER DEVICE: eligibility for the one-dispatch path is decided
// per device (one group, a small result), so on a context over several devices some shards may have gone direct and
// others through the streaming kernels + an asynchronous copy — a device is only excused from the stream wait when
// every doorbell it owes has rung (a bell that stays silent for a millisecond falls back to the wait as well).
int32_t wait_devices(ProbeCall &c)
{
    bsg_ctx *ctx = c.ctx;
    std::vector<uint8_t> rang(c.nd, 0);
    for (const DirectResult &p : c.direct)
        rang[p.di] = p.wait(std::chrono::microseconds(1000)) ? std::max<uint8_t>(rang[p.di], 1) : 2;     // 2: a bell of this device stayed silent
    for (uint32_t di = 0; di < c.nd; ++di) {
        if (rang[di] == 1) continue;                                          // every result of this device is in host memory
        Device &d = *ctx->devs[di];
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) return rc;
        if (ctx->spin_wait_us) {   // a short busy-wait first: waking from a blocking wait costs more than a single query's kernels run
            const auto t0 = std::chrono::steady_clock::now();
            while (hipStreamQuery(d.stream) == hipErrorNotReady &&
                   std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(ctx->spin_wait_us)) {}
        }
        HIP_TRY(hipStreamSynchronize(d.stream));
        if (d.copy_stream) HIP_TRY(hipStreamSynchronize(d.copy_stream));
        d.copy_busy[0] = d.copy_busy[1] = false;
    }
    return BSG_OK;
}

int32_t probe_arenas(bsg_ctx *ctx, const std::vector<std::shared_ptr<Arena>> &arenas, const Batch &B, uint32_t flags,
                     uint64_t *out_survivors, uint64_t *out_dev, uint32_t *rows_hdr)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const uint32_t n_arenas = (uint32_t)arenas.size();
    if (B.n_queries == 0 || n_arenas == 0) return BSG_OK;
    ProbeCall c{ctx, arenas, B, flags, out_survivors, out_dev, rows_hdr, nd, n_arenas};
    c.packed = (flags & BSG_PROBE_ROWS_PACKED) != 0;
    if (rows_hdr) {
        if (c.packed)
            for (auto &a : arenas)
                for (auto &sh : a->shards)
                    if ((sh.n_blocks + 63) / 64 > bsg::kRowsStageG)
                        return fail(BSG_E_UNSUPPORTED, "BSG_PROBE_ROWS_PACKED takes arenas of at most %u blocks per device (one of these holds %u)",
                                    bsg::kRowsStageG * 64, sh.n_blocks);
        c.RL = rows_layout(arenas, nd, B.n_queries);
        if (int32_t rc = rows_targets(ctx, arenas, B, out_survivors, out_dev, rows_hdr, c.d_rows, c.d_hdr, c.packed)) return rc;
    } else if (c.packed) {
        return fail(BSG_E_INVALID, "BSG_PROBE_ROWS_PACKED is a flag of bsg_probe_many_rows");
    }
    if (!B.subs.empty()) return probe_composite(ctx, arenas, B, flags, out_survivors, out_dev);
    c.timed = flags & BSG_PROBE_TIMED;
    // Fusing pays while a dispatch is short enough for its ramp + completion to matter (a few arenas); behind a large
    // group the evaluation workgroups only take LDS and issue slots from the streaming (measured at 20-32 arenas of
    // 35 MB per dispatch: fused 5.9 us per arena, k_probe_terms + k_eval_programs 5.2 + 1.0 us with the evaluation
    // costing no HBM time of its own).
    c.fuse = !(flags & BSG_PROBE_NOFUSE) && !B.many_terms && B.n_kinds > 0 && 2 * bsg::eval_lds_bytes(B.max_cw, B.max_depth) <= 64 * 1024;
    c.fuse_max_arenas = std::min(ctx->fuse_max_arenas, bsg::kMaxFusedArenas);
    c.limit = std::max(1u, std::min(ctx->group_limit, bsg::kMaxExtGroupArenas));
    c.out_off = bsh::survivor_offsets(n_arenas, B.n_queries, ArenaBlocks{arenas});
    c.parts.resize(nd > 1 && out_survivors && !rows_hdr ? nd : 0);
    for (uint32_t di = 0; di < nd; ++di) if (int32_t rc = enqueue_device(c, di)) return rc;      // every device before any wait
    if (flags & BSG_PROBE_ASYNC) return BSG_OK;
    if (int32_t rc = wait_devices(c)) return rc;
    for (DirectResult &p : c.direct) {
        memcpy(p.dst, p.buf, p.bytes);
        p.drained = true;                          // the doorbell rang, or the stream was waited for
    }
    if (!c.parts.empty()) {
        memset(out_survivors, 0, c.out_off[n_arenas] * 8);
        for (uint32_t di = 0; di < nd; ++di)
            bsh::merge_device_part(c.parts[di].data(), n_arenas, ShardBlocks{arenas, di}, ArenaBlocks{arenas}, B.n_queries, di, nd, out_survivors, c.out_off.data());
    }
    return BSG_OK;
}

}  // namespace

extern "C" int32_t bsg_set_timed_stride(bsg_ctx *ctx, uint32_t stride)
{
    BSG_ENTER(ctx);
    ctx->timed_stride = stride ? stride : 1;
    ctx->timed_counter = 0;
    return BSG_OK;
}

extern "C" int32_t bsg_set_probe_group(bsg_ctx *ctx, uint32_t max_arenas_per_launch)
{
    BSG_ENTER(ctx);
    ctx->group_limit = max_arenas_per_launch ? std::min(max_arenas_per_launch, bsg::kMaxExtGroupArenas) : 1024u;
    return BSG_OK;
}

// lab knobs (tools/, bench sweeps, tests of the paths the defaults no longer take): key 1 = compaction rounds of the
// many-term probe mode; key 2 = bytes of HBM a binned build of a large bitset may use for its locations (0: global atomics);
// key 3 = most distinct terms of a small batch that takes the one-dispatch path k_probe_direct (0: never);
// key 4 = pieces bsg_arena_load_sections decodes a region in (1: one launch after the whole copy);
// key 6 = fewest locations (entries x k) for which a bitset beyond LDS is built from binned locations (default 4 M);
// key 7 = fewest entries of a bsg_hash_entries / bsg_build* call that is cut into one part per device (default 256 K);
// key 8 = fewest row bytes of a bsg_ingest_rows / bsg_match_rows call that is cut into one part per device (default 8 MiB);
// key 9 = 1: the file-level union goes through global hash tables (round 2's path) instead of LDS partitions; key 10 = start the
// partitioned union with 2^value x too few partitions (exercises its retry and its fallback; 32 + v: 2^v x too many — runs of a few, one, less than one home slot)
extern "C" int32_t bsg_set_lab(bsg_ctx *ctx, uint32_t key, uint64_t value)
{
    BSG_ENTER(ctx);
    if (key == 1) { ctx->compact_rounds = (uint32_t)std::min<uint64_t>(value, 16); return BSG_OK; }
    if (key == 2) { ctx->bin_scratch_bytes = value; return BSG_OK; }
    if (key == 6) { ctx->bin_min_locs = value; return BSG_OK; }
    if (key == 3) { ctx->direct_max_terms = (uint32_t)std::min<uint64_t>(value, 192); return BSG_OK; }
    if (key == 4) { ctx->load_pieces = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(value, 1), 64); return BSG_OK; }
    if (key == 7) { ctx->shard_min_entries = value; return BSG_OK; }
    if (key == 8) { ctx->shard_min_row_bytes = value; return BSG_OK; }
    if (key == 9) { ctx->union_mode = (uint32_t)std::min<uint64_t>(value, 1); return BSG_OK; }
    if (key == 11) { ctx->fold_helpers = (uint32_t)std::min<uint64_t>(value, 64); return BSG_OK; }
    if (key == 10) { ctx->union_coarsen = (uint32_t)std::min<uint64_t>(value, 56); return BSG_OK; }
    // keys 12-14: the combiner of concurrent bsg_query calls (combine_api.inc): 12 = 0 every call goes alone / 1 calls that meet share
    // dispatches (default); 13 = cycles in flight (default 2);
    // 15 (tests) = (linger microseconds << 16) | calls: a collector waits that long, or until that many calls are queued, before it collects;
    // 16 = queries asked of one arena in a cycle from which the arena is streamed once for all of them (default 8, 0 = never); 17 = microseconds a
    // queued caller polls before it sleeps (default 60); 19 = percent of a single-group device-resident run whose evaluation moves to a second
    // stream beside the rest's probe (0 = off); 26 = 0: few-term launches never take k_probe_gather (default 1); 27 = chunks a single gathered group is probed in, its evaluation
    // under its own gather (k_gather_fused; 0 = bsh::pipeline_chunks decides, 1 = never, n >= 2 = n chunks, + (percent of an equal share for the last chunk) << 16, + (1 = evaluation workgroups in front, 2 = spread) << 24);
    // 28 = workgroups of the gather kernels per CU (0 = bsh::kGatherWorkgroupsPerCu, above 4 = no cap)
    if (key == 12) { ctx->cmb.mode = (uint32_t)std::min<uint64_t>(value, 2); return BSG_OK; }
    if (key == 13) { ctx->cmb.sync.max_inflight = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(value, 1), 8); return BSG_OK; }
    if (key == 15) { ctx->cmb.linger_us = (uint32_t)std::min<uint64_t>(value >> 16, 1000000); ctx->cmb.linger_calls = (uint32_t)(value & 0xFFFF); return BSG_OK; }
    if (key == 20) { ctx->cmb.profile = value ? 1u : 0u; return BSG_OK; }
    if (key == 19) { ctx->tail_split_pct = (uint32_t)std::min<uint64_t>(value, 95); return BSG_OK; }
    if (key == 16) { ctx->cmb.hot_min_queries = (uint32_t)std::min<uint64_t>(value, 1u << 20); return BSG_OK; }
    if (key == 25) { ctx->cmb.wait_spin_us = (uint32_t)std::min<uint64_t>(value, 1000000); return BSG_OK; }
    if (key == 24) { ctx->cmb.part_bytes = std::max<uint64_t>(value, 8); return BSG_OK; }
    if (key == 22) { ctx->solo_ring_wgs = (uint32_t)std::min<uint64_t>(value, 1u << 30); return BSG_OK; }
    if (key == 21) { ctx->cmb.inline_jobs = value ? 1u : 0u; return BSG_OK; }
    if (key == 26) { ctx->gather_kernel = value ? 1u : 0u; return BSG_OK; }     // 0: launches never take k_probe_gather (tools/probe_gather_lab.py: the per-block gathered path of k_probe_terms on its own)
    if (key == 28) { ctx->gather_wgs_per_cu = (uint32_t)std::min<uint64_t>(value, 255); return BSG_OK; }     // workgroups of the gather kernels per CU, by an LDS pad (bsh::gather_lds_pad): 0 = the planner's rule, 1-4, above 4 = no cap
    if (key == 27) { ctx->pipeline_key = value & 0xFFFFFFFFull; return BSG_OK; }     // 0: bsh::pipeline_chunks decides, 1: never, n (+ last-chunk percent << 16, + placement << 24): n chunks
    if (key == 29) { ctx->partition_hash_mask = value ? 3u : 0xFFFFFFFFu; return BSG_OK; }     // 1: the partition dictionary's hash keeps its low 2 bits (partition.hip.h: the byte compare and the collision rounds, on purpose)
    if (key == 17) { ctx->cmb.sync.spin_us = (uint32_t)std::min<uint64_t>(value, 1000000); return BSG_OK; }
    return fail(BSG_E_INVALID, "unknown lab key %u", key);
}

extern "C" int32_t bsg_set_ingest_chunk(bsg_ctx *ctx, uint64_t bytes)
{
    BSG_ENTER(ctx);
    ctx->ingest_chunk_bytes = bytes ? std::max<uint64_t>(bytes, 1u << 16) : (64ull << 20);
    return BSG_OK;
}

extern "C" int32_t bsg_set_spin_wait(bsg_ctx *ctx, uint32_t microseconds)
{
    BSG_ENTER(ctx);
    ctx->spin_wait_us = microseconds;
    return BSG_OK;
}

extern "C" int32_t bsg_set_fuse_limit(bsg_ctx *ctx, uint32_t max_arenas)
{
    BSG_ENTER(ctx);
    ctx->fuse_max_arenas = max_arenas;
    return BSG_OK;
}

extern "C" int32_t bsg_set_gather_cost(bsg_ctx *ctx, uint32_t bytes_per_probe)
{
    BSG_ENTER(ctx);
    ctx->gather_cost = bytes_per_probe;
    return BSG_OK;
}

extern "C" int32_t bsg_lab_last_probe_route(bsg_ctx *ctx, uint32_t *out_route)
{
    BSG_ENTER(ctx);
    if (!out_route) return fail(BSG_E_INVALID, "null argument");
    *out_route = ctx->last_probe_route.load(std::memory_order_relaxed);
    return BSG_OK;
}

extern "C" int32_t bsg_probe_batch(bsg_ctx *ctx, uint64_t arena_id, uint64_t batch_id, uint32_t flags, uint64_t *out_survivors)
{
    BSG_ENTER(ctx);
    std::vector<std::shared_ptr<Arena>> arenas(1);
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_arena(ctx, arena_id, arenas[0])) return rc;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    if ((flags & BSG_PROBE_ASYNC) && out_survivors)
        return fail(BSG_E_INVALID, "BSG_PROBE_ASYNC cannot return survivors to the host");
    return probe_arenas(ctx, arenas, *batch, flags, out_survivors, nullptr);
}

extern "C" int32_t bsg_probe_many(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, uint32_t flags,
                                  uint64_t *out_survivors)
{
    BSG_ENTER(ctx);
    if (n_arenas && !arena_ids) return fail(BSG_E_INVALID, "null argument");
    if ((flags & BSG_PROBE_ASYNC) && out_survivors && ctx->devs.size() != 1)
        return fail(BSG_E_INVALID, "BSG_PROBE_ASYNC with a host output needs a single-device context (shards are interleaved on the host)");
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    std::vector<std::shared_ptr<Arena>> arenas(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena(ctx, arena_ids[i], arenas[i])) return rc;
    // without an output pointer the call only enqueues (round-1 contract: pair with bsg_sync)
    return probe_arenas(ctx, arenas, *batch, out_survivors ? flags : (flags | BSG_PROBE_ASYNC), out_survivors, nullptr);
}

extern "C" int32_t bsg_probe_many_rows(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, uint32_t flags,
                                       uint64_t *out_rows, uint32_t *out_hdr)
{
    BSG_ENTER(ctx);
    if ((n_arenas && !arena_ids) || !out_rows || !out_hdr) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    std::vector<std::shared_ptr<Arena>> arenas(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena(ctx, arena_ids[i], arenas[i])) return rc;
    return probe_arenas(ctx, arenas, *batch, flags, out_rows, nullptr, out_hdr);
}

extern "C" int32_t bsg_survivor_row_list(uint32_t hdr, const uint64_t *row, uint32_t n_blocks, uint32_t *out_blocks, uint32_t cap, uint32_t *out_n)
{
    if (!out_n || (cap && !out_blocks)) return fail(BSG_E_INVALID, "null argument");
    const uint32_t tag = hdr >> 30, cnt = hdr & 0x3FFFFFFFu;
    *out_n = cnt;
    if (cnt > n_blocks) return fail(BSG_E_INVALID, "row header counts %u survivors of %u blocks", cnt, n_blocks);
    if (cnt > cap) return fail(BSG_E_INVALID, "the row holds %u surviving blocks, the buffer %u", cnt, cap);
    if (tag == bsg::kRowNone) return BSG_OK;
    if (tag == bsg::kRowAll) {
        if (cnt != n_blocks) return fail(BSG_E_INVALID, "an ALL row header counts %u of %u blocks", cnt, n_blocks);    // (cap >= cnt was checked)
        for (uint32_t b = 0; b < n_blocks; ++b) out_blocks[b] = b;
        return BSG_OK;
    }
    if (!row) return fail(BSG_E_INVALID, "null row");
    if (tag == bsg::kRowList) {
        // a LIST row lives in the row's dense slot: at most 2 * ceil(n_blocks / 64) ids, ascending and below n_blocks
        if (cnt > 2 * ((n_blocks + 63) / 64)) return fail(BSG_E_INVALID, "a LIST row header counts %u ids, the row's slot holds %u", cnt, 2 * ((n_blocks + 63) / 64));
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(row);
        for (uint32_t i = 0; i < cnt; ++i)
            if (ids[i] >= n_blocks || (i && ids[i] <= ids[i - 1])) return fail(BSG_E_INVALID, "a LIST row's ids are not ascending block numbers below %u", n_blocks);
        memcpy(out_blocks, ids, (size_t)cnt * 4);
        return BSG_OK;
    }
    uint32_t n = 0;
    if (int32_t rc = bsg_survivor_list(row, n_blocks, out_blocks, cap, &n)) return rc;
    if (n != cnt) return fail(BSG_E_INVALID, "a DENSE row header counts %u survivors, its words hold %u", cnt, n);
    return BSG_OK;
}

// The surviving blocks of (arena, query) in GLOBAL block order from the rows bsg_probe_many_rows left in the caller's buffers: on a
// context of nd devices the nd shards' rows (local numbers, each ascending) are merged — global = local * nd + device; NONE shards
// contribute nothing, ALL shards every block they hold, neither touches the row's payload.
static int32_t survivor_rows_list_impl(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, const uint64_t *rows,
                                       const uint32_t *hdr, uint32_t arena_index, uint32_t query, uint32_t *out_blocks, uint32_t cap, uint32_t *out_n,
                                       bool packed)
{
    if ((n_arenas && !arena_ids) || !rows || !hdr || !out_n || (cap && !out_blocks)) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    if (arena_index >= n_arenas || query >= batch->n_queries) return fail(BSG_E_INVALID, "row (%u, %u) outside %u arenas x %u queries", arena_index, query, n_arenas, batch->n_queries);
    std::vector<std::shared_ptr<Arena>> arenas(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena(ctx, arena_ids[i], arenas[i])) return rc;
    const uint32_t nd = (uint32_t)ctx->devs.size(), Q = batch->n_queries;
    const RowsLayout L = rows_layout(arenas, nd, Q);
    // every shard's row expanded to its ascending local list (NONE / ALL without looking at the slot), then the nd-way merge
    std::vector<std::vector<uint32_t>> local(nd);
    uint64_t total = 0;
    for (uint32_t d = 0; d < nd; ++d) {
        const uint32_t nl = arenas[arena_index]->shards[d].n_blocks;
        if (nl == 0) continue;
        const uint32_t G = (nl + 63) / 64;
        uint32_t h = packed ? 0u : hdr[((size_t)d * n_arenas + arena_index) * Q + query];
        const uint64_t *row = rows + L.row_base[d] + L.arena_off[d][arena_index] + (uint64_t)query * G;
        if (packed) {
            // byte headers (tag << 6 | a LIST row's count); the run of 256 queries this one belongs to: payloads back to back from the
            // run's first slot, in query order
            // (the same answer as bsg_probe_many_rows gave for these arenas: no packed rows of them were ever written)
            if (G > bsg::kRowsStageG) return fail(BSG_E_UNSUPPORTED, "packed rows hold arenas of at most %u blocks per device", bsg::kRowsStageG * 64);
            const uint32_t q0 = query & ~255u;
            const uint8_t *hr = reinterpret_cast<const uint8_t *>(hdr) + ((size_t)d * n_arenas + arena_index) * Q + q0;
            uint64_t off = 0;
            for (uint32_t j = 0; j < query - q0; ++j) {
                const uint32_t tg = hr[j] >> 6, cn = hr[j] & 63u;
                if (tg == bsg::kRowList) { if (cn > 2u * G) return fail(BSG_E_INVALID, "a LIST row header counts %u ids, a row holds %u", cn, 2u * G); off += (cn + 1u) >> 1; }
                else if (tg == bsg::kRowDense) off += G;
            }
            row = rows + L.row_base[d] + L.arena_off[d][arena_index] + (uint64_t)q0 * G + off;
            const uint32_t tg = hr[query - q0] >> 6;
            uint32_t cn = hr[query - q0] & 63u;
            if (tg == bsg::kRowAll) cn = nl;
            else if (tg == bsg::kRowDense) { cn = 0; for (uint32_t g = 0; g < G; ++g) cn += (uint32_t)__builtin_popcountll(row[g]); }
            else if (tg == bsg::kRowNone) cn = 0;
            h = (tg << 30) | cn;
        }
        // (a stale or garbage header must not size an allocation: a count beyond the shard's blocks is left to bsg_survivor_row_list's
        //  own validation, which answers BSG_E_INVALID)
        local[d].resize(std::min<uint32_t>(h & 0x3FFFFFFFu, nl));
        uint32_t n = 0;
        if (int32_t rc = bsg_survivor_row_list(h, row, nl, local[d].data(), (uint32_t)local[d].size(), &n)) return rc;
        total += n;
    }
    *out_n = (uint32_t)total;
    if (total > cap) return fail(BSG_E_INVALID, "the row holds %llu surviving blocks, the buffer %u", (unsigned long long)total, cap);
    if (nd == 1) { if (total) memcpy(out_blocks, local[0].data(), total * 4); return BSG_OK; }
    std::vector<size_t> at(nd, 0);
    for (uint64_t o = 0; o < total; ++o) {
        uint32_t best = 0; uint64_t best_g = ~0ull;
        for (uint32_t d = 0; d < nd; ++d)
            if (at[d] < local[d].size()) { const uint64_t g = (uint64_t)local[d][at[d]] * nd + d; if (g < best_g) { best_g = g; best = d; } }
        out_blocks[o] = (uint32_t)best_g;
        ++at[best];
    }
    return BSG_OK;
}

extern "C" int32_t bsg_survivor_rows_list(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, const uint64_t *rows,
                                          const uint32_t *hdr, uint32_t arena_index, uint32_t query, uint32_t *out_blocks, uint32_t cap, uint32_t *out_n)
{
    BSG_ENTER(ctx);
    return survivor_rows_list_impl(ctx, arena_ids, n_arenas, batch_id, rows, hdr, arena_index, query, out_blocks, cap, out_n, false);
}

// ... from rows written with BSG_PROBE_ROWS_PACKED
extern "C" int32_t bsg_survivor_rows_list_packed(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, const uint64_t *rows,
                                                 const uint32_t *hdr, uint32_t arena_index, uint32_t query, uint32_t *out_blocks, uint32_t cap, uint32_t *out_n)
{
    BSG_ENTER(ctx);
    return survivor_rows_list_impl(ctx, arena_ids, n_arenas, batch_id, rows, hdr, arena_index, query, out_blocks, cap, out_n, true);
}

// Words / headers bsg_probe_many_rows writes for these arenas and this batch on this context (what out_rows / out_hdr must hold).
extern "C" int32_t bsg_survivor_rows_size(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, uint64_t *out_row_words, uint64_t *out_hdr_words)
{
    BSG_ENTER(ctx);
    if ((n_arenas && !arena_ids) || !out_row_words || !out_hdr_words) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    std::vector<std::shared_ptr<Arena>> arenas(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena(ctx, arena_ids[i], arenas[i])) return rc;
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const RowsLayout L = rows_layout(arenas, nd, batch->n_queries);
    *out_row_words = L.row_base[nd];
    *out_hdr_words = (uint64_t)nd * n_arenas * batch->n_queries;
    return BSG_OK;
}

extern "C" int32_t bsg_probe_many_dev(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, uint32_t flags,
                                      void *d_out_survivors)
{
    BSG_ENTER(ctx);
    if ((n_arenas && !arena_ids) || !d_out_survivors) return fail(BSG_E_INVALID, "null argument");
    if (ctx->devs.size() != 1) return fail(BSG_E_UNSUPPORTED, "bsg_probe_many_dev needs a single-device context");
    std::shared_ptr<Batch> batch;
    if (int32_t rc = get_batch(ctx, batch_id, batch)) return rc;
    std::vector<std::shared_ptr<Arena>> arenas(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena(ctx, arena_ids[i], arenas[i])) return rc;
    return probe_arenas(ctx, arenas, *batch, flags, nullptr, static_cast<uint64_t *>(d_out_survivors));
}

extern "C" {

int32_t bsg_probe(bsg_ctx *ctx, uint64_t arena_id, const bsg_term *terms, uint32_t n_terms, const uint32_t *prog_ops,
                  const uint32_t *prog_off, uint32_t n_queries, uint64_t *out_survivors)
{
    BSG_ENTER(ctx);
    if (n_queries && !out_survivors) return fail(BSG_E_INVALID, "out_survivors is null");
    uint64_t bid = 0;
    if (int32_t rc = bsg_batch_create(ctx, terms, n_terms, prog_ops, prog_off, n_queries, &bid)) return rc;
    const int32_t rc = bsg_probe_batch(ctx, arena_id, bid, 0, out_survivors);
    const std::string saved = rc ? g_err : std::string();
    (void)bsg_batch_free(ctx, bid);
    if (rc) fail(rc, "%s", saved.c_str());   // the probe's message, not the free's
    return rc;
}

}  // extern "C"

namespace {

// A small query set laid out for the one-dispatch kernels: k_query_direct's kernel arguments, an entry of a k_query_jobs table.
// Terms grouped by kind without padding (<= 16: one verdict word), programs lowered over those positions, op j of query q at
// prog[j * n_queries + q].  fits == false: beyond 16 terms / 128 program words / the interpreter's LDS stack — not an error.
struct CompactQuery {
    bool fits = false;
    uint32_t n_kinds = 0, kind[3] = {0, 0, 0}, term_begin[3] = {0, 0, 0}, term_count[3] = {0, 0, 0};
    uint32_t len = 1, stride = 0, max_depth = 1;
    uint8_t pos_term[bsg::kQueryMaxTerms];      // position -> index of the term in the call's own list
    uint64_t th[4 * bsg::kQueryMaxTerms];
    uint32_t prog[bsg::kQueryMaxProgWords];
};

int32_t compact_query(const std::vector<bsg_term> &terms, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, CompactQuery &c)
{
    const uint32_t n_terms = (uint32_t)terms.size();
    c.fits = false;
    if (n_terms > bsg::kQueryMaxTerms || n_queries > bsg::kEvalThreads) return BSG_OK;
    uint32_t count[3] = {0, 0, 0}, begin[3] = {0, 0, 0}, fill[3] = {0, 0, 0};
    for (uint32_t t = 0; t < n_terms; ++t) count[terms[t].kind]++;
    uint32_t cursor = 0;
    for (uint32_t k = 0; k < 3; ++k) {
        if (!count[k]) continue;
        c.kind[c.n_kinds] = k; c.term_begin[c.n_kinds] = cursor; c.term_count[c.n_kinds] = count[k];
        begin[k] = cursor; cursor += count[k]; c.n_kinds++;
    }
    memset(c.th, 0, sizeof c.th);
    std::vector<uint32_t> term_pos(n_terms);
    for (uint32_t t = 0; t < n_terms; ++t) {
        const uint32_t pos = begin[terms[t].kind] + fill[terms[t].kind]++;
        term_pos[t] = pos;
        c.pos_term[pos] = (uint8_t)t;
        for (int j = 0; j < 4; ++j) c.th[(size_t)j * bsg::kQueryMaxTerms + pos] = terms[t].h[j];
    }
    std::vector<std::vector<uint32_t>> lowered(n_queries);
    uint32_t Lmax = 1;
    for (uint32_t i = 0; i < n_queries; ++i) {
        if (prog_off[i + 1] < prog_off[i]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", i);
        const uint32_t n_ops = prog_off[i + 1] - prog_off[i];
        if (n_ops && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
        uint32_t depth = 1;
        if (int32_t rc = lower_program(prog_ops + prog_off[i], n_ops, n_terms, term_pos, lowered[i], depth)) return rc;
        c.max_depth = std::max(c.max_depth, depth);
        Lmax = std::max<uint32_t>(Lmax, (uint32_t)lowered[i].size());
    }
    if ((uint64_t)Lmax * n_queries > bsg::kQueryMaxProgWords || bsg::direct_lds_bytes(1, c.max_depth) > 64 * 1024) return BSG_OK;
    for (uint32_t w = 0; w < bsg::kQueryMaxProgWords; ++w) c.prog[w] = 7u << 28;
    for (uint32_t i = 0; i < n_queries; ++i)
        for (size_t j = 0; j < lowered[i].size(); ++j) c.prog[j * n_queries + i] = lowered[i][j];      // TERM arg = position = verdict slot
    c.len = Lmax; c.stride = n_queries;
    c.fits = true;
    return BSG_OK;
}

// ---- one interactive Query() in ONE call: strings in, survivors out (direct.hip.h: k_query_direct) ----
// The call by itself (no other caller to share a dispatch with: combine_api.inc): terms already hashed, arenas resolved.
// cq: the call's compact layout when the caller has it already.
int32_t query_solo(bsg_ctx *ctx, const std::vector<std::shared_ptr<Arena>> &arenas, const std::vector<bsg_term> &terms,
                   const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, uint64_t *out_survivors, const CompactQuery *cq = nullptr)
{
    const uint32_t n_arenas = (uint32_t)arenas.size(), n_terms = (uint32_t)terms.size();
    const uint32_t nd = (uint32_t)ctx->devs.size();
    // ---- does the call fit one dispatch per device with everything in the kernel arguments? ----
    CompactQuery local;
    if (!cq) { if (int32_t rc = compact_query(terms, prog_ops, prog_off, n_queries, local)) return rc; cq = &local; }
    bool fast = cq->fits;
    for (uint32_t di = 0; di < nd && fast; ++di) {
        uint32_t n = 0;
        for (auto &a : arenas) n += a->shards[di].n_blocks ? 1u : 0u;
        if (n > bsg::kQueryMaxArenas) fast = false;
    }
    bsg::QueryKernArgs q{};
    const uint32_t max_depth = cq->max_depth;
    if (fast) {
        q.a.n_kinds = cq->n_kinds;
        for (uint32_t y = 0; y < 3; ++y) { q.a.kind[y] = cq->kind[y]; q.a.term_begin[y] = cq->term_begin[y]; q.a.term_count[y] = cq->term_count[y]; }
        memcpy(q.th, cq->th, sizeof q.th);
        memcpy(q.prog, cq->prog, sizeof q.prog);
        q.len = cq->len; q.stride = n_queries;
        q.a.Tp = bsg::kQueryMaxTerms; q.a.Wt = 1; q.a.n_queries = n_queries; q.a.Lmax = cq->len; q.a.max_depth = max_depth;
    }
    if (!fast) {                                        // a larger batch: the batch object after all (hashes still from the host)
        uint64_t bid = 0;
        if (int32_t rc = bsg_batch_create(ctx, terms.data(), n_terms, prog_ops, prog_off, n_queries, &bid)) return rc;
        std::shared_ptr<Batch> batch;
        int32_t rc = get_batch(ctx, bid, batch);
        if (!rc) rc = probe_arenas(ctx, arenas, *batch, 0, out_survivors, nullptr);
        const std::string saved = rc ? g_err : std::string();
        (void)bsg_batch_free(ctx, bid);
        if (rc) fail(rc, "%s", saved.c_str());
        return rc;
    }
    // ---- one k_query_direct per device that holds blocks; survivors land in page-locked memory, a doorbell says when ----
    std::vector<DirectResult> pend;
    for (uint32_t di = 0; di < nd; ++di) {
        Device &d = *ctx->devs[di];
        Group g;
        for (uint32_t i = 0; i < n_arenas; ++i) if (arenas[i]->shards[di].n_blocks) group_add(g, n_queries, 1, arenas[i]->shards[di], i);
        if (g.shards.empty()) continue;
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) return rc;
        pend.emplace_back();
        DirectResult &p = pend.back();
        if (int32_t rc = p.take(d, di, g.out_words * 8)) return rc;
        bsg::QueryKernArgs k = q;
        k.a.n_arenas = (uint32_t)g.shards.size();
        // the kernel's own doorbell costs every workgroup a system-scope fence, and those serialise: beyond a few dozen workgroups
        // (one query over ten 1 000-block files: 160) a one-thread dispatch behind the kernel rings instead
        const bool ring = (uint64_t)g.max_G * k.a.n_arenas > ctx->solo_ring_wgs;
        k.a.out = p.buf;
        if (!ring) { k.a.done_count = d.d_direct_count; k.a.flag = p.flag; k.a.seq = p.seq; }
        fill_refs(g, k.t.ar);
        hipLaunchKernelGGL(bsg::k_query_direct, dim3(g.max_G, 1, k.a.n_arenas), dim3(bsg::kEvalThreads), bsg::direct_lds_bytes(1, max_depth), d.stream, k);
        HIP_TRY(hipGetLastError());
        if (ring) if (int32_t rc = ring_doorbell(d, p.flag, p.seq)) return rc;
    }
    for (DirectResult &p : pend)
        if (!p.wait(std::chrono::microseconds(1000))) {     // the bell did not ring within a millisecond: ask the runtime, on this buffer's device only
            std::lock_guard<std::mutex> lk(p.dev->mu);
            if (int32_t rc = use_device(*p.dev)) return rc;
            HIP_TRY(hipStreamSynchronize(p.dev->stream));
        }
    for (DirectResult &p : pend) p.drained = true;
    if (nd == 1) {
        // one device: a group's arenas are the caller's non-empty arenas in order, their words back to back — as out_survivors wants them
        if (!pend.empty()) memcpy(out_survivors, pend[0].buf, pend[0].bytes);
        return BSG_OK;
    }
    const std::vector<uint64_t> out_off = bsh::survivor_offsets(n_arenas, n_queries, ArenaBlocks{arenas});
    memset(out_survivors, 0, out_off[n_arenas] * 8);
    for (const DirectResult &p : pend)
        bsh::merge_device_part(p.buf, n_arenas, ShardBlocks{arenas, p.di}, ArenaBlocks{arenas}, n_queries, p.di, nd, out_survivors, out_off.data());
    return BSG_OK;
}

}  // namespace
