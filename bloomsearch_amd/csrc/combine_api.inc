// combine_api.inc — bsg_query and the COMBINER behind it (included by bloomgpu.hip after probe_api.inc).
//
// The reference probes per file from concurrent workers: every candidate file of a Query() is consulted by a goroutine of its own
// (query_exec.go:303-357, 427-431; up to MaxQueryConcurrency = 1 000 of them), and several Query() calls run at once.  Mirrored
// literally — one bsg_query per (query, file) — those calls serialise on the device's stream at one ~8 us dispatch each and the
// batched kernels are never reached (SURVEY 7, hard part 5: batching is the crux).  The combiner forms the batch INSIDE the library,
// from whoever is calling at the moment — no caller waits for a window to fill:
//   * a call that finds the device idle and nobody queued goes alone, at once: exactly the old one-dispatch path (k_query_direct);
//   * a call that arrives while another is collecting or in flight queues itself.  When the device side frees up, the HEAD of the
//     queue is appointed collector: it takes everything queued and splits it into (call, arena) PAIRS.
//       - an arena asked enough in this cycle (8 three-term queries per 35 KB of filters per block: run_cycle) is a "hot file": its callers' query sets become ONE batch (each distinct term
//         hashed and probed once) and the arena is STREAMED once for all of them — k_probe_terms + k_eval_programs, the 0.85-of-HBM
//         kernels of the batch API;
//       - every other pair is a JOB of one k_query_jobs dispatch (direct.hip.h): the gather regime, cost proportional to the pairs
//         asked for — the reference's own pattern (one query, one call per candidate file) is a list of such jobs.
//     One table upload and one dispatch (pair) per hot arena, one for the whole job list, survivors written straight into
//     page-locked memory; the collector hands its role to the next head (the next cycle is prepared while this one runs: two in
//     flight), waits for its own cycle, and deals every caller its rows.
// Results are those of the solo path bit for bit (tests/test_concurrency_gpu.py, tools/fuzz_probe.py): the same programs over the
// same verdict bits, only computed together.  bsg_set_lab key 12 = 0 turns combining off.
#include <ctime>
#include <unordered_map>
#include "host/combiner_sync.hpp"

namespace {

struct QReq : bsgsync::Waiter {
    // the call
    std::vector<std::shared_ptr<Arena>> arenas;
    std::vector<bsg_term> terms;
    const uint32_t *prog_ops = nullptr, *prog_off = nullptr;
    uint32_t n_queries = 0;
    uint64_t *out = nullptr;
    // prepared on the caller's own thread (the collector only copies and re-indexes)
    CompactQuery cq;                              // the layout of the one-dispatch kernels (k_query_direct, a job of k_query_jobs)
    std::vector<uint64_t> out_off;                // arena j's rows start at out + out_off[j]
    int32_t rc = BSG_OK;
    std::string err;
};

constexpr uint32_t kCmbCallQueries = 64, kCmbCallArenas = 32;   // larger calls (and calls beyond the compact layout) go alone
constexpr uint64_t kCmbCallBytes = 1ull << 20;                  // ... and calls with more than 1 MB of survivor rows (64 queries x 32 arenas of 4 000 blocks)

using bsgsync::release_role;
using bsgsync::release_slot;

struct TermKey {
    uint64_t h[4]; uint32_t kind;
    bool operator==(const TermKey &o) const { return kind == o.kind && h[0] == o.h[0] && h[1] == o.h[1] && h[2] == o.h[2] && h[3] == o.h[3]; }
};
struct TermKeyHash { size_t operator()(const TermKey &k) const { return (size_t)(k.h[0] ^ (k.h[1] * 0x9E3779B97F4A7C15ULL) ^ k.kind); } };

struct Pair { QReq *r; uint32_t j; };                                  // call r's arena at position j of its list

// what one device was handed for one unit of a cycle (a hot arena's batch, or the job list)
struct Dispatch {
    uint32_t di = 0;
    Device *dev = nullptr;
    void *d_block = nullptr;                                            // the unit's table in device memory (pool)
    std::pair<uint64_t *, size_t> stage{nullptr, 0}, result{nullptr, 0};
    uint64_t *flag = nullptr; uint64_t seq = 0;                         // the doorbell behind the dispatch (k_ring): the last word of `result`
    bool enqueued = false, copied = false;
    CmbSet set;                                                         // where d_block / stage / result come from and go back to
    std::vector<std::pair<Pair, uint64_t>> rows;                        // every pair served here and the first word of its rows in `result`
};

// One hot arena of a cycle: the query sets of the calls that ask it, as ONE batch.
struct Hot {
    std::vector<std::shared_ptr<Arena>> arenas;                         // one hot arena — or all of a cycle's, probed by ONE dispatch (run_cycle)
    std::vector<Pair> pairs;
    std::vector<uint32_t> pair_call;                                    // pairs[i] belongs to calls[pair_call[i]]
    std::vector<uint32_t> pair_arena;                                   // ... and asks arenas[pair_arena[i]]
    std::vector<QReq *> calls;                                          // distinct calls, in order of first appearance
    std::vector<uint32_t> q0;                                           // first query of calls[i] in the batch
    Batch B;
    BatchTables T;
    bool planned = false;
};

inline uint32_t call_terms(const CompactQuery &c)                     // distinct terms of a call (its kinds' segments lie back to back)
{
    return c.n_kinds ? c.term_begin[c.n_kinds - 1] + c.term_count[c.n_kinds - 1] : 0u;
}

// the distinct terms of the bucket's calls (a term shared by several calls is probed once) and all their programs
int32_t plan_hot(Hot &h)
{
    std::unordered_map<TermKey, uint32_t, TermKeyHash> index;
    std::vector<bsg_term> terms;
    std::vector<std::vector<uint32_t>> lowered;
    uint32_t max_depth = 1, q0 = 0;
    h.q0.clear();
    for (QReq *rp : h.calls) {
        const QReq &r = *rp;
        h.q0.push_back(q0);
        uint32_t local[bsg::kQueryMaxTerms];
        for (size_t t = 0; t < r.terms.size(); ++t) {
            TermKey k{{r.terms[t].h[0], r.terms[t].h[1], r.terms[t].h[2], r.terms[t].h[3]}, r.terms[t].kind};
            auto it = index.find(k);
            if (it == index.end()) { it = index.emplace(k, (uint32_t)terms.size()).first; terms.push_back(r.terms[t]); }
            local[t] = it->second;
        }
        // the call's programs as its compact layout holds them (op j of query q at prog[j * n_queries + q], NOP padded, TERM argument
        // = position): positions -> the call's terms -> the bucket's terms
        for (uint32_t q = 0; q < r.n_queries; ++q) {
            lowered.emplace_back();
            std::vector<uint32_t> &prog = lowered.back();
            for (uint32_t j = 0; j < r.cq.len; ++j) {
                uint32_t op = r.cq.prog[j * r.n_queries + q];
                if ((op >> 28) == 7u) continue;
                if ((op >> 28) == 0u) op = local[r.cq.pos_term[op & 0x0FFFFFFFu]];
                prog.push_back(op);
            }
        }
        max_depth = std::max(max_depth, r.cq.max_depth);
        q0 += r.n_queries;
    }
    bool too_big = false;
    if (int32_t rc = plan_batch_tables(terms.data(), (uint32_t)terms.size(), lowered, max_depth, h.B, h.T, &too_big)) return rc;
    h.planned = true;
    return BSG_OK;
}

// Registers a dispatch on device di and takes its scratch — a set {device block, page-locked stage, page-locked result} from the
// device's cache of such sets (a lock of its own, held for the push / pop only: giving scratch back never waits for the device
// lock the next collector holds while it enqueues), grown under d.mu (held by the caller) when too small.
int32_t open_dispatch(Device &d, uint32_t di, size_t table_bytes, uint64_t result_words, std::vector<Dispatch> &all, Dispatch **out)
{
    all.emplace_back();
    Dispatch &P = all.back();
    P.di = di; P.dev = &d;
    {
        std::lock_guard<std::mutex> lk(d.cmb_mu);
        if (!d.cmb_sets.empty()) { P.set = d.cmb_sets.back(); d.cmb_sets.pop_back(); }
    }
    auto pow2 = [](size_t n) { size_t c = 256 * 1024; while (c < n) c <<= 1; return c; };
    if (P.set.d_cap < table_bytes) {
        if (P.set.d_block) (void)hipFree(P.set.d_block);
        P.set.d_block = nullptr; P.set.d_cap = 0;
        if (hipMalloc(&P.set.d_block, pow2(table_bytes)) != hipSuccess) return fail(BSG_E_NOMEM, "no device memory for a combined table of %zu bytes", table_bytes);
        P.set.d_cap = pow2(table_bytes);
    }
    auto grow = [&](std::pair<uint64_t *, size_t> &b, size_t need) -> int32_t {
        if (b.second >= need) return BSG_OK;
        if (b.first) (void)hipHostFree(b.first);
        b = {nullptr, 0};
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b.first), pow2(need), hipHostMallocDefault));
        b.second = pow2(need);
        return BSG_OK;
    };
    if (int32_t rc = grow(P.set.stage, table_bytes)) return rc;
    if (int32_t rc = grow(P.set.result, result_words * 8 + 64)) return rc;
    P.d_block = P.set.d_block; P.stage = P.set.stage; P.result = P.set.result;
    *out = &P;
    return BSG_OK;
}

// the doorbell behind a dispatch's kernels (the word behind its `words` result words); under d.mu
int32_t ring_behind(Device &d, Dispatch &P, uint64_t words)
{
    P.flag = P.result.first + words; P.seq = ++d.direct_seq;
    *reinterpret_cast<volatile uint64_t *>(P.flag) = 0;
    return ring_doorbell(d, P.flag, P.seq);
}

// A hot arena on one device: tables up (one copy), k_probe_terms + k_eval_programs, survivors straight into page-locked memory.
int32_t enqueue_hot(bsg_ctx *ctx, Hot &h, uint32_t di, std::vector<Dispatch> &all)
{
    Device &d = *ctx->devs[di];
    const Batch &B = h.B;
    Group g;
    std::vector<int64_t> at(h.arenas.size(), -1);                       // arena -> first word of its rows [n_queries][G] in the result
    std::vector<uint32_t> G_of(h.arenas.size(), 0);
    uint64_t gp = 0;
    for (size_t pos = 0; pos < h.arenas.size(); ++pos) {
        const ArenaShard &s = h.arenas[pos]->shards[di];
        if (s.n_blocks == 0) continue;
        group_add(g, B.n_queries, B.Wt, s, (uint32_t)pos);
        at[pos] = (int64_t)(gp * B.n_queries);
        G_of[pos] = (s.n_blocks + 63) / 64;
        gp += G_of[pos];
    }
    if (g.shards.empty()) return BSG_OK;
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    Dispatch *Pp = nullptr;
    if (int32_t rc = open_dispatch(d, di, h.T.total, g.out_words, all, &Pp)) return rc;
    Dispatch &P = *Pp;
    h.T.pack_into(reinterpret_cast<uint8_t *>(P.stage.first));
    P.copied = true;
    HIP_TRY(hipMemcpyAsync(P.d_block, P.stage.first, h.T.total, hipMemcpyHostToDevice, d.stream));
    const BatchDev bd = h.T.dev_at(static_cast<uint8_t *>(P.d_block));
    if (int32_t rc = enqueue_terms(ctx, d, g, bd, B, 0, nullptr)) return rc;
    if (int32_t rc = enqueue_eval(d, g, bd, B, 0, nullptr, P.result.first)) return rc;
    if (int32_t rc = ring_behind(d, P, g.out_words)) return rc;
    for (size_t i = 0; i < h.pairs.size(); ++i) {
        const uint32_t pa = h.pair_arena[i];
        if (at[pa] >= 0) P.rows.emplace_back(h.pairs[i], (uint64_t)at[pa] + (uint64_t)h.q0[h.pair_call[i]] * G_of[pa]);
    }
    P.enqueued = true;
    return BSG_OK;
}

// The job list on one device: every pair whose arena holds blocks there is a job; the calls' hashes and programs follow the records
// in one table (a call's jobs share them).
int32_t enqueue_jobs(bsg_ctx *ctx, const std::vector<Pair> &pairs, uint32_t di, std::vector<Dispatch> &all)
{
    Device &d = *ctx->devs[di];
    std::vector<bsg::QJob> jobs;
    std::vector<Pair> job_pair;
    struct Blob { const QReq *r; uint32_t at; };                         // a call's hashes + programs: byte offset behind the records
    std::vector<Blob> blobs;
    uint32_t wg = 0, max_depth = 1, blob_bytes = 0;
    uint64_t words = 0;
    jobs.reserve(pairs.size()); job_pair.reserve(pairs.size());
    for (const Pair &p : pairs) {
        const ArenaShard &s = p.r->arenas[p.j]->shards[di];
        if (s.n_blocks == 0) continue;
        const CompactQuery &c = p.r->cq;
        const uint32_t nt = call_terms(c);
        const uint32_t stride = std::max(nt, 1u);
        if (blobs.empty() || blobs.back().r != p.r) {                   // (a call's pairs follow each other)
            blobs.push_back(Blob{p.r, blob_bytes});
            blob_bytes += (4 * stride * 8 + c.len * p.r->n_queries * 4 + 7) / 8 * 8;
        }
        bsg::QJob J{};
        J.words = s.d_words; J.desc = s.d_desc; J.n_blocks = s.n_blocks; J.wg0 = wg;
        J.out_off = words;
        J.th_off = blobs.back().at;                                     // (turned into table offsets below)
        J.th_stride = stride;
        J.n_queries = (uint16_t)p.r->n_queries; J.len = (uint16_t)c.len; J.max_depth = (uint16_t)c.max_depth; J.n_kinds = (uint16_t)c.n_kinds;
        for (uint32_t y = 0; y < 3; ++y) { J.kind[y] = (uint8_t)c.kind[y]; J.term_begin[y] = (uint8_t)c.term_begin[y]; J.term_count[y] = (uint8_t)c.term_count[y]; }
        jobs.push_back(J);
        job_pair.push_back(p);
        const uint32_t G = (s.n_blocks + 63) / 64;
        wg += G;
        words += (uint64_t)p.r->n_queries * G;
        max_depth = std::max(max_depth, c.max_depth);
    }
    if (jobs.empty()) return BSG_OK;
    // table: [jobs][per call: th (4 rows of its terms, u64) | prog (len x n_queries u32)][the job of every workgroup, u32] — ~120 bytes
    // for a 3-term query
    const size_t blobs_at = jobs.size() * sizeof(bsg::QJob);
    const size_t wg_at = blobs_at + blob_bytes;
    const size_t table = wg_at + (size_t)wg * 4;
    for (auto &J : jobs) {
        const size_t at = blobs_at + J.th_off;
        J.th_off = (uint32_t)(at / 8);
        J.prog_off = (uint32_t)((at + (size_t)4 * J.th_stride * 8) / 4);
    }
    // a short list's table travels in the kernel arguments (k_query_jobs_inline): nothing uploaded in front of the dispatch (16 callers
    // on one arena: enqueue 19.4 -> 11.3 us per cycle, 3.2 -> 4.3 x 10^5 queries/s; over 12 arenas 3.6 -> 4.1)
    const uint32_t inl = table <= bsg::kJobsInlineBytes ? ctx->cmb.inline_jobs : 0u;
    bsg::JobsInlineArgs ia;
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    Dispatch *Pp = nullptr;
    if (int32_t rc = open_dispatch(d, di, inl ? 0 : table, words, all, &Pp)) return rc;
    Dispatch &P = *Pp;
    uint8_t *st = inl ? ia.table : reinterpret_cast<uint8_t *>(P.stage.first);
    memcpy(st, jobs.data(), blobs_at);
    for (const Blob &b : blobs) {
        const CompactQuery &c = b.r->cq;
        const uint32_t nt = call_terms(c), stride = std::max(nt, 1u);
        uint64_t *th = reinterpret_cast<uint64_t *>(st + blobs_at + b.at);
        for (uint32_t j = 0; j < 4; ++j) for (uint32_t t = 0; t < stride; ++t) th[j * stride + t] = c.th[j * bsg::kQueryMaxTerms + t];
        memcpy(th + 4 * stride, c.prog, (size_t)c.len * b.r->n_queries * 4);
    }
    {
        uint32_t *wj = reinterpret_cast<uint32_t *>(st + wg_at);
        for (size_t i = 0; i < jobs.size(); ++i) {
            const uint32_t w1 = i + 1 < jobs.size() ? jobs[i + 1].wg0 : wg;
            for (uint32_t w = jobs[i].wg0; w < w1; ++w) wj[w] = (uint32_t)i;
        }
    }
    // completion by a doorbell dispatch BEHIND the kernel, not k_query_direct's own doorbell: that costs every WORKGROUP a
    // system-scope fence (an L2 write-back) before it may count itself done — 16 of them for one call, thousands for a job list,
    // where they serialise (measured: 570 jobs 10.2 ms; for the short lists of 16 callers the kernel's own doorbell saves 3 us of
    // enqueueing and adds 3-5 us of waiting: 3.4 vs 4.3 x 10^5 queries/s).  The end of the kernel releases its writes to the host anyway.
    bsg::JobsArgs &a = ia.a;
    a = bsg::JobsArgs{};
    a.out = P.result.first;
    a.n_jobs = (uint32_t)jobs.size(); a.n_wg = wg;
    a.wg_at = (uint32_t)wg_at;
    P.copied = true;                                  // from here on something of this dispatch may be on the stream: a failure below must drain it before the scratch is reused
    if (inl) {
        hipLaunchKernelGGL(bsg::k_query_jobs_inline, dim3(wg), dim3(bsg::kEvalThreads), bsg::direct_lds_bytes(1, max_depth), d.stream, ia);
    } else {
        HIP_TRY(hipMemcpyAsync(P.d_block, st, table, hipMemcpyHostToDevice, d.stream));
        a.jobs = static_cast<const bsg::QJob *>(P.d_block);
        a.tab = static_cast<const uint64_t *>(P.d_block);
        a.wg_job = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(P.d_block) + wg_at);
        hipLaunchKernelGGL(bsg::k_query_jobs, dim3(wg), dim3(bsg::kEvalThreads), bsg::direct_lds_bytes(1, max_depth), d.stream, a);
    }
    HIP_TRY(hipGetLastError());
    if (int32_t rc = ring_behind(d, P, words)) return rc;
    for (size_t i = 0; i < jobs.size(); ++i) P.rows.emplace_back(job_pair[i], jobs[i].out_off);
    P.enqueued = true;
    return BSG_OK;
}

// Wait for a cycle's dispatches, deal the rows, give the scratch back.  rc_in / msg_in: the cycle already failed (only wait + free).
int32_t finish_dispatches(bsg_ctx *ctx, std::vector<Dispatch> &all, int32_t rc_in, const std::string &msg_in, uint64_t *ns_wait)
{
    int32_t rc = rc_in;
    std::string msg = msg_in;
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const auto t_w = std::chrono::steady_clock::now();
    // How long to poll: a cycle's doorbell rings 15-300 us after the enqueue on an otherwise idle device (16 callers on one arena ...
    // 256 callers x 10 arenas with hot arenas streamed), and being woken from a blocking wait costs tens of microseconds — a fixed 50 us
    // put every large cycle to sleep and cost the 256-caller points a third of their rate.  So: 4 x the running mean of the waits that
    // ended while polling, within [50 us, 1 ms]; a device busy with somebody else's milliseconds outlasts that and the collector sleeps.
    Combiner &cm = ctx->cmb;
    const uint64_t spin_ns = cm.wait_spin_us ? (uint64_t)cm.wait_spin_us * 1000u
                                             : std::min<uint64_t>(std::max<uint64_t>(4ull * cm.wait_ema_ns.load(std::memory_order_relaxed), 50000u), 1000000u);
    for (auto &P : all) {
        bool done = !P.enqueued && !P.copied;           // nothing of this dispatch was put on the stream
        if (P.enqueued && P.flag) {
            const auto t0 = std::chrono::steady_clock::now();
            uint64_t waited = 0;
            for (uint32_t i = 0; __atomic_load_n(P.flag, __ATOMIC_ACQUIRE) != P.seq; ++i) {
                bsgsync::cpu_relax();
                if ((i & 63) == 63 && (waited = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count()) > spin_ns) break;
            }
            done = __atomic_load_n(P.flag, __ATOMIC_ACQUIRE) == P.seq;
            if (done) {
                waited = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                const uint32_t ema = cm.wait_ema_ns.load(std::memory_order_relaxed);
                cm.wait_ema_ns.store((uint32_t)((7ull * ema + std::min<uint64_t>(waited, 1000000u)) / 8u), std::memory_order_relaxed);
            }
        }
        if (!done) {
            // ... then SLEEP: the stream is busy with somebody else's work (a 28 ms k_ingest_rows of the flush worker on this device turned
            // every combined query of round 5 into a 20 ms busy-wait on a quota-limited box).  An event recorded on the stream NOW lies
            // behind this dispatch — and behind a failed enqueue's earlier copies —, created with hipEventBlockingSync so that the wait
            // costs no processor time; no device lock is held while waiting (the next collector keeps enqueueing).
            (void)hipSetDevice(P.dev->id);
            hipError_t e = hipSuccess;
            if (!P.set.drained) e = hipEventCreateWithFlags(&P.set.drained, hipEventBlockingSync | hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(P.set.drained, P.dev->stream);
            if (e == hipSuccess) e = hipEventSynchronize(P.set.drained);
            else {                                        // no event to be had: drain the stream the old way before the scratch is reused
                std::lock_guard<std::mutex> lk(P.dev->mu);
                e = hipStreamSynchronize(P.dev->stream);
            }
            if (e != hipSuccess && !rc) { rc = BSG_E_HIP; msg = std::string("combined dispatch failed: ") + hipGetErrorString(e); }
            if (e == hipSuccess && P.enqueued && P.flag && __atomic_load_n(P.flag, __ATOMIC_ACQUIRE) != P.seq && !rc) {
                rc = BSG_E_HIP; msg = "combined dispatch finished without ringing its doorbell";
            }
        }
    }
    *ns_wait += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_w).count();
    const auto t_s = std::chrono::steady_clock::now();
    if (!rc) {
        for (const auto &P : all)
            for (const auto &row : P.rows) {
                QReq &r = *row.first.r;
                const Arena &A = *r.arenas[row.first.j];
                const ArenaShard &s = A.shards[P.di];
                const uint64_t G = (s.n_blocks + 63) / 64;
                const uint64_t *src = P.result.first + row.second;
                uint64_t *dst = r.out + r.out_off[row.first.j];
                if (nd == 1) memcpy(dst, src, (size_t)r.n_queries * G * 8);
                else bsh::interleave_shard(src, r.n_queries, s.n_blocks, P.di, nd, dst, ((uint64_t)A.n_blocks + 63) / 64);      // (the caller zeroed its rows)
            }
    }
    ctx->cmb.ns_scatter.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_s).count(), std::memory_order_relaxed);
    const auto t_f = std::chrono::steady_clock::now();
    for (auto &P : all) {
        std::lock_guard<std::mutex> lk(P.dev->cmb_mu);
        P.dev->cmb_sets.push_back(P.set);
    }
    all.clear();
    ctx->cmb.ns_free.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_f).count(), std::memory_order_relaxed);
    if (rc) g_err = msg;
    return rc;
}

int32_t query_solo_req(bsg_ctx *ctx, QReq &r)
{
    return query_solo(ctx, r.arenas, r.terms, r.prog_ops, r.prog_off, r.n_queries, r.out, &r.cq);
}

// Another caller's request served alone on this thread: its failure is ITS failure (message carried over, not recorded on this
// thread's scope).
void serve_alone(bsg_ctx *ctx, QReq &r, bool mine)
{
    bsg_ctx *saved = tl_scope;
    if (!mine) tl_scope = nullptr;
    r.rc = query_solo_req(ctx, r);
    if (r.rc) r.err = g_err;
    tl_scope = saved;
}

// The collector's cycle: the caller holds the role and a cycle slot (bsgsync::submit / kick).
void run_cycle(bsg_ctx *ctx, QReq &me)
{
    Combiner &c = ctx->cmb;
    std::vector<QReq *> cyc;
    if (c.linger_us) {            // lab (bsg_set_lab key 15): the collector waits for company, so that tests meet every merge shape on purpose
        const auto t0 = std::chrono::steady_clock::now();
        auto waiting = [&]() {    // (the holder of the role may walk the stacks: nobody else takes from them)
            uint32_t n = 1;
            for (uint32_t k = 0; k < bsgsync::kStacks; ++k)
                for (bsgsync::Waiter *w = c.sync.head[k].p.load(std::memory_order_acquire); w; w = w->next) n += w != &me;
            return n;
        };
        while (waiting() < c.linger_calls && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(c.linger_us)) std::this_thread::yield();
    }
    bsgsync::drain(c.sync, me, cyc);      // everything that waits, the collector in front
    c.n_cycles.fetch_add(1, std::memory_order_relaxed);
    c.n_cycle_calls.fetch_add(cyc.size(), std::memory_order_relaxed);
    {
        uint64_t m = c.max_cycle_calls.load(std::memory_order_relaxed);
        while (m < cyc.size() && !c.max_cycle_calls.compare_exchange_weak(m, cyc.size(), std::memory_order_relaxed)) {}
    }
    const uint32_t hot_min = c.hot_min_queries;
    // the role covers the taking of the calls only: the next collector may take what arrives from now on while this cycle is
    // prepared, enqueued and run (as many cycles at a time as there are slots)
    release_role(c.sync);
    auto retire = [&]() { release_slot(c.sync); };
    if (cyc.size() == 1) {
        serve_alone(ctx, me, true);
        c.n_solo.fetch_add(1, std::memory_order_relaxed);
        release_slot(c.sync);
        return;
    }
    auto since = [](std::chrono::steady_clock::time_point a) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - a).count(); };
    uint64_t n_disp = 0, n_hot = 0, ns_prepare = 0, ns_enq = 0, ns_wait = 0, ns_deal = 0;
    bsg_ctx *saved_scope = tl_scope;
    tl_scope = nullptr;                                     // a shared failure is every caller's, reported by each on its own thread
    // one part of the cycle: pair, plan, enqueue, wait, deal
    auto serve_part = [&](const std::vector<QReq *> &part, std::vector<Dispatch> &all) {
        const auto t_start = std::chrono::steady_clock::now();
        // ---- the cycle's (call, arena) pairs; arenas asked many queries become hot buckets, the rest the job list ----
        // arena -> distinct terms asked of it in this cycle, call by call (x its blocks = the bit-test chains a gather would run)
        std::unordered_map<const Arena *, uint64_t> asked;
        for (QReq *r : part) {
            const uint32_t nt = call_terms(r->cq);
            for (auto &a : r->arenas) asked[a.get()] += nt;
        }
        // a cycle short enough for its whole job table to ride in the kernel arguments stays a job list whatever it asks: one dispatch
        // without an upload beats table + stream + evaluation (16 callers on one arena: 3.3 -> 4.6 x 10^5 calls/s) while the list is that short
        bool short_list = c.inline_jobs != 0;
        if (short_list) {
            size_t bytes = 0;
            for (QReq *r : part) {
                const CompactQuery &q = r->cq;
                const uint32_t nt = std::max(call_terms(q), 1u);
                bytes += (4 * nt * 8 + q.len * r->n_queries * 4 + 7) / 8 * 8;
                for (auto &a : r->arenas) bytes += sizeof(bsg::QJob) + 4 * (((size_t)a->n_blocks + 63) / 64);
                if (bytes > bsg::kJobsInlineBytes) { short_list = false; break; }
            }
        }
        // Stream or gather?  A (block, term) test by gather costs ~6 scattered sector reads at 52 x 10^9/s, a streamed byte 1 / 6.8 TB/s:
        // by device time alone a test is worth ~800 streamed bytes; measured on C2's arena (35 KB of filters per block, 3-term queries;
        // thresholds of 4 / 8 / 12 / 24 queries) the best threshold is 8 queries = 1 465 bytes per test, table upload and planning
        // included.  Scaled by the arena's own bytes per block, so that 8 queries never stream an arena of 1 MB filters (64 blocks:
        // 67 MB for 1 500 tests) and 2 queries do stream one of 1 KB filters.
        auto is_hot = [&](const Arena *a) {
            if (!hot_min || short_list) return false;
            uint64_t words = 0;
            for (const ArenaShard &sh : a->shards) words += sh.n_words;
            return asked[a] * (uint64_t)a->n_blocks * 35160u >= words * 8 * 3 * hot_min;
        };
        std::unordered_map<const Arena *, uint32_t> hot_of;
        std::vector<std::shared_ptr<Arena>> hot_arenas;
        struct HotPair { Pair p; uint32_t arena; };
        std::vector<HotPair> hot_pairs;                         // in call order (a call's pairs follow each other)
        std::vector<Pair> job_pairs;
        uint64_t hot_G = 0, hot_queries = 0;
        for (QReq *r : part) {
            bool any_hot = false;
            for (uint32_t j = 0; j < r->arenas.size(); ++j) {
                const Arena *a = r->arenas[j].get();
                if (a->n_blocks == 0) continue;
                if (is_hot(a)) {
                    auto it = hot_of.find(a);
                    if (it == hot_of.end()) {
                        it = hot_of.emplace(a, (uint32_t)hot_arenas.size()).first;
                        hot_arenas.push_back(r->arenas[j]);
                        hot_G += ((uint64_t)a->n_blocks + 63) / 64;
                    }
                    hot_pairs.push_back(HotPair{Pair{r, j}, it->second});
                    any_hot = true;
                } else job_pairs.push_back(Pair{r, j});
            }
            if (any_hot) hot_queries += r->n_queries;
        }
        // Several hot arenas: ONE batch of all their callers' queries probed against all of them by one dispatch pair — every hot arena is
        // streamed once either way; what the product adds is evaluation and result rows nobody asked for (cheap while small), what it
        // saves is a table upload + two dispatches + the planning per arena (measured, 256 callers x 10 arenas each: 5-6 hot arenas per
        // cycle cost the collector 230 us of planning + enqueueing).  A product beyond 4 MB of rows, or more arenas than one dispatch's
        // kernel arguments hold, goes arena by arena.
        const bool merged = hot_arenas.size() > 1 && hot_arenas.size() <= bsg::kMaxGroupArenas && hot_queries * hot_G * 8 <= (4ull << 20);
        std::vector<Hot> hots(hot_arenas.empty() ? 0 : (merged ? 1 : hot_arenas.size()));
        if (merged) hots[0].arenas = hot_arenas;
        else for (size_t i = 0; i < hot_arenas.size(); ++i) hots[i].arenas.assign(1, hot_arenas[i]);
        for (const HotPair &hp : hot_pairs) {
            Hot &h = hots[merged ? 0 : hp.arena];
            if (h.calls.empty() || h.calls.back() != hp.p.r) h.calls.push_back(hp.p.r);
            h.pairs.push_back(hp.p);
            h.pair_call.push_back((uint32_t)h.calls.size() - 1);
            h.pair_arena.push_back(merged ? hp.arena : 0u);
        }
        const uint32_t nd = (uint32_t)ctx->devs.size();
        all.reserve((hots.size() + 1) * nd);                    // (open_dispatch hands out pointers into it)
        int32_t rc = BSG_OK;
        uint64_t enq = 0;
        for (Hot &h : hots) {
            if (rc) break;
            rc = plan_hot(h);
            if (rc == BSG_E_UNSUPPORTED) {                      // beyond one launch's limits as a batch: its pairs are jobs after all
                rc = BSG_OK;
                job_pairs.insert(job_pairs.end(), h.pairs.begin(), h.pairs.end());
                continue;
            }
            const auto t1 = std::chrono::steady_clock::now();
            for (uint32_t di = 0; di < nd && !rc; ++di) rc = enqueue_hot(ctx, h, di, all);
            enq += since(t1);
        }
        {
            const auto t1 = std::chrono::steady_clock::now();
            for (uint32_t di = 0; di < nd && !rc; ++di) rc = enqueue_jobs(ctx, job_pairs, di, all);
            enq += since(t1);
        }
        const std::string msg = rc ? g_err : std::string();
        ns_prepare += since(t_start) - enq; ns_enq += enq;  // pairing + planning | enqueueing
        n_disp += all.size(); n_hot += hot_arenas.size();
        const auto t_wait = std::chrono::steady_clock::now();
        uint64_t waited = 0;
        rc = finish_dispatches(ctx, all, rc, msg, &waited);
        ns_wait += waited; ns_deal += since(t_wait) - waited;
        const std::string fmsg = rc ? g_err : std::string();
        for (QReq *r : part) { r->rc = rc; if (rc) r->err = fmsg; }
    };
    // A std::bad_alloc out of the part's vectors / maps / plan_hot must not unwind past the cycle: its callers sleep in their futexes
    // until release_cycle, and the cycle slot is one of two (ADVICE r5).  The part fails for every one of its calls instead; whatever
    // was enqueued is drained before its scratch goes back.
    auto serve = [&](const std::vector<QReq *> &part) {
        std::vector<Dispatch> all;
        try {
            serve_part(part, all);
        } catch (const std::exception &ex) {
            const std::string m = std::string("combined cycle failed: ") + ex.what();
            uint64_t waited = 0;
            try { (void)finish_dispatches(ctx, all, BSG_E_NOMEM, m, &waited); } catch (...) {}
            for (QReq *r : part) { r->rc = BSG_E_NOMEM; r->err = m; }
        }
    };
    // the rows of a cycle lie in page-locked scratch the device keeps: a cycle asking for more than Combiner::part_bytes of them (hundreds of
    // callers with calls near kCmbCallBytes) is served in parts, one after the other
    uint64_t bytes = 0;
    for (QReq *r : cyc) bytes += r->out_off.back() * 8;
    const uint64_t part_bytes = c.part_bytes;
    if (bytes <= part_bytes) serve(cyc);
    else {
        std::vector<QReq *> part;
        for (size_t i0 = 0; i0 < cyc.size();) {
            size_t i1 = i0;
            uint64_t b = 0;
            while (i1 < cyc.size() && (i1 == i0 || b + cyc[i1]->out_off.back() * 8 <= part_bytes)) b += cyc[i1++]->out_off.back() * 8;
            try { part.assign(cyc.begin() + i0, cyc.begin() + i1); }
            catch (const std::exception &) { for (size_t i = i0; i < i1; ++i) { cyc[i]->rc = BSG_E_NOMEM; cyc[i]->err = "combined cycle failed: out of memory"; } i0 = i1; continue; }
            serve(part);
            i0 = i1;
        }
    }
    tl_scope = saved_scope;
    const auto t_ret = std::chrono::steady_clock::now();
    retire();
    c.ns_retire.fetch_add(since(t_ret), std::memory_order_relaxed);
    const auto t_wake = std::chrono::steady_clock::now();
    bsgsync::release_cycle(cyc);
    c.n_dispatches.fetch_add(n_disp, std::memory_order_relaxed);
    c.n_hot.fetch_add(n_hot, std::memory_order_relaxed);
    c.ns_prepare.fetch_add(ns_prepare, std::memory_order_relaxed); c.ns_enqueue.fetch_add(ns_enq, std::memory_order_relaxed);
    c.ns_wait.fetch_add(ns_wait, std::memory_order_relaxed);
    c.ns_deal.fetch_add(ns_deal + since(t_ret), std::memory_order_relaxed);      // rows dealt out + callers released
    c.ns_wake.fetch_add(since(t_wake), std::memory_order_relaxed);
}

uint64_t thread_cpu_ns()
{
    timespec ts;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

int32_t combiner_submit(bsg_ctx *ctx, QReq &r)
{
    Combiner &c = ctx->cmb;
    // lab (bsg_set_lab key 20): the caller's own processor time around the wait — what a call costs the host besides the collector's work
    bsgsync::PhaseClock pc;
    pc.now = thread_cpu_ns;
    const bool prof = c.profile != 0;
    const uint64_t cpu0 = prof ? thread_cpu_ns() : 0;
    bsgsync::submit(c.sync, r, [ctx](QReq &me) { run_cycle(ctx, me); }, prof ? &pc : nullptr);
    if (prof) {
        c.ns_cpu_call.fetch_add(thread_cpu_ns() - cpu0, std::memory_order_relaxed); c.n_cpu_calls.fetch_add(1, std::memory_order_relaxed);
        c.ns_cpu_wait.fetch_add(pc.wait, std::memory_order_relaxed); c.ns_cpu_duty.fetch_add(pc.duty, std::memory_order_relaxed);
        c.ns_cpu_collect.fetch_add(pc.collect, std::memory_order_relaxed);
    }
    if (r.rc) return fail(r.rc, "%s", r.err.c_str());
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_query(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, const uint8_t *term_bytes, const uint32_t *term_off,
                  const uint32_t *term_kinds, uint32_t n_terms, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                  uint64_t *out_survivors)
{
    BSG_ENTER(ctx);
    if (n_arenas && !arena_ids) return fail(BSG_E_INVALID, "arena_ids is null");
    if (n_queries && (!prog_off || !out_survivors)) return fail(BSG_E_INVALID, "null argument");
    if (n_terms && (!term_off || !term_kinds)) return fail(BSG_E_INVALID, "terms are null");
    for (uint32_t t = 0; t < n_terms; ++t) {
        if (term_off[t + 1] < term_off[t]) return fail(BSG_E_INVALID, "term_off not monotone at %u", t);
        if (term_kinds[t] > 2) return fail(BSG_E_INVALID, "term %u has unknown kind %u", t, term_kinds[t]);
    }
    if (n_terms && term_off[n_terms] && !term_bytes) return fail(BSG_E_INVALID, "term_bytes is null");
    if (n_queries == 0 || n_arenas == 0) return BSG_OK;
    // the probed strings are hashed HERE, on the caller's thread, by the function the kernels hash entries with (TestString hashes
    // inside the call too, query_exec.go:141-154): no device launch for a handful of strings
    QReq r;
    r.terms.resize(n_terms);
    for (uint32_t t = 0; t < n_terms; ++t) {
        bsg::base_hashes(term_bytes + term_off[t], term_off[t + 1] - term_off[t], r.terms[t].h);
        r.terms[t].kind = term_kinds[t];
        r.terms[t].reserved = 0;
    }
    r.arenas.resize(n_arenas);
    for (uint32_t i = 0; i < n_arenas; ++i) if (int32_t rc = get_arena_cached(ctx, arena_ids[i], r.arenas[i])) return rc;
    r.prog_ops = prog_ops; r.prog_off = prog_off; r.n_queries = n_queries; r.out = out_survivors;
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
        if (prog_off[q + 1] > prog_off[q] && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    }
    // the layout of the one-dispatch kernels, on the caller's thread (in parallel with every other caller)
    if (int32_t rc = compact_query(r.terms, prog_ops, prog_off, n_queries, r.cq)) return rc;
    if (ctx->cmb.mode == 2) return BSG_OK;                 // lab (key 12 = 2): the caller's own preparation only, nothing probed
    r.out_off.resize(n_arenas + 1, 0);
    for (uint32_t i = 0; i < n_arenas; ++i) r.out_off[i + 1] = r.out_off[i] + (uint64_t)n_queries * (((uint64_t)r.arenas[i]->n_blocks + 63) / 64);
    if (ctx->cmb.mode == 0 || !r.cq.fits || n_queries > kCmbCallQueries || n_arenas > kCmbCallArenas || r.out_off[n_arenas] * 8 > kCmbCallBytes)
        return query_solo_req(ctx, r);
    if (ctx->devs.size() > 1) memset(out_survivors, 0, r.out_off[n_arenas] * 8);          // shards' bits are OR-ed in
    return combiner_submit(ctx, r);
}

// lab: out[0..4] = profiled calls, ns of callers' processor time per phase summed: whole call, push + wait (incl. the futex), wake duty,
// collecting (a collector's whole cycle)
int32_t bsg_lab_query_cpu(bsg_ctx *ctx, uint64_t *out, int32_t reset)
{
    BSG_ENTER(ctx);
    Combiner &c = ctx->cmb;
    std::atomic<uint64_t> *src[] = {&c.n_cpu_calls, &c.ns_cpu_call, &c.ns_cpu_wait, &c.ns_cpu_duty, &c.ns_cpu_collect};
    for (int i = 0; i < 5; ++i) out[i] = reset ? src[i]->exchange(0) : src[i]->load();
    return BSG_OK;
}

int32_t bsg_query_stats_read(bsg_ctx *ctx, bsg_query_stats *out, int32_t reset)
{
    BSG_ENTER(ctx);
    if (!out) return fail(BSG_E_INVALID, "out is null");
    Combiner &c = ctx->cmb;
    std::atomic<uint64_t> *src[] = {&c.n_cycle_calls, &c.n_solo, &c.n_cycles, &c.n_cycle_calls, &c.n_dispatches, &c.n_hot, &c.max_cycle_calls,
                                    &c.ns_prepare, &c.ns_enqueue, &c.ns_wait, &c.ns_deal, &c.ns_wake, &c.ns_scatter, &c.ns_free, &c.ns_retire};
    uint64_t *dst[] = {&out->calls, &out->solo_calls, &out->cycles, &out->cycle_calls, &out->dispatches, &out->hot_arenas, &out->max_calls_per_cycle,
                       &out->ns_prepare, &out->ns_enqueue, &out->ns_wait, &out->ns_deal, &out->ns_wake, &out->ns_scatter, &out->ns_free, &out->ns_retire};
    for (size_t i = 1; i < sizeof src / sizeof *src; ++i) *dst[i] = reset ? src[i]->exchange(0) : src[i]->load();
    out->calls = out->cycle_calls;                 // every eligible call is served by a cycle (a cycle of one when it goes alone)
    return BSG_OK;
}

}  // extern "C"
