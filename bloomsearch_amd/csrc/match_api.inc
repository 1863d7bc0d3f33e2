// match_api.inc — C-ABI of the device row matcher (included by bloomgpu.hip).  Kernel: match.hip.h.

namespace {

static_assert(bsh_rxg::kMaxRegexConds == bsg::kRxMaxConds && bsh_rxg::kSingleLdsCap == bsg::kRxLdsCap && bsh_rxg::kManyLdsCap == bsg::kRxManyLdsCap &&
                  bsh_rxg::kSingleSlots == bsg::kRxActive && (bsh_rxg::kManySlots == bsg::kRxManyActive || BSG_RX_MANY_SLOTS != 4) &&
                  bsh_rxg::kPathCap == bsg::kPathCap,
              "host/regex_groups.hpp states the kernels' limits");

// The LDS table blob of a call's FieldRegex conditions (layout: match.hip.h; built by host/regex_groups.hpp).  BSG_E_UNSUPPORTED,
// before anything is launched, for a pattern outside the compiler's subset, more than kRxMaxConds of them, or tables over `cap`
// (kRxLdsCap; kRxManyLdsCap for the batched call, whose blob also holds the conditions' user masks: users [n_conds], else NULL).
int32_t build_rx_blob(const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                      std::vector<uint32_t> &blob, uint32_t &n_rx, uint32_t cap = bsg::kRxLdsCap, const uint64_t *users = nullptr)
{
    const bsh_rxg::BlobResult r = bsh_rxg::build_blob(cond_bytes, cond_off, cond_kinds, n_conds, BSG_KIND_FIELD_REGEX, cap, users, blob);
    n_rx = r.n_rx;
    switch (r.status) {
    case bsh_rxg::BlobStatus::Ok: return BSG_OK;
    case bsh_rxg::BlobStatus::TooMany:
        return fail(BSG_E_UNSUPPORTED, "%u regex conditions (the device matcher holds %u)", n_rx, bsg::kRxMaxConds);
    case bsh_rxg::BlobStatus::Pattern: {
        const uint32_t c = r.cond;
        const std::string_view pat((const char *)cond_bytes + cond_off[2 * c + 1], cond_off[2 * c + 2] - cond_off[2 * c + 1]);
        return fail(BSG_E_UNSUPPORTED, "regex condition %u (pattern \"%.*s\"): %s", c, (int)std::min<size_t>(pat.size(), 200), pat.data(), r.err.c_str());
    }
    default: return fail(BSG_E_UNSUPPORTED, "regex tables need more than %u bytes of LDS", cap);
    }
}

// bsg_match_rows_many: what a part needs beyond the single call's arguments.  `prog` then holds the lowered programs of all
// queries behind each other and out_bits n_queries planes of call_words words.
struct ManyPlan {
    std::vector<uint32_t> prog_off;        // [n_queries + 1] into prog
    const uint32_t *set_first_row;         // the call's set table (n_sets == 0: every query on every row)
    const uint64_t *set_mask;
    uint32_t n_sets, n_queries;
    size_t call_words;
};

// rows [r0, r1) (r0 a multiple of 64: whole words of out_bits) on one device; fb receives the GLOBAL indices of the rows handed back
// many: the batched call (k_match_rows_many*; with regex conditions k_match_rows_many_regex*), NULL = one expression
int32_t match_rows_on(bsg_ctx *ctx, Device &d, const uint8_t *rows, const uint64_t *row_off, uint32_t r0, uint32_t r1,
                      const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds, uint32_t cond_len,
                      const std::vector<uint32_t> &prog, const std::vector<uint32_t> &rx_blob, uint32_t n_rx, const bsg::TokSpec *tok,
                      uint64_t *out_bits, std::vector<uint32_t> &fb, float *ms, const ManyPlan *many = nullptr)
{
    const uint32_t n_rows = r1 - r0;
    const uint64_t byte0 = row_off[r0], n_bytes = row_off[r1] - byte0;
    const LabTrace trace{many ? (n_rx ? "bsg_match_rows_many_regex" : "bsg_match_rows_many") : "bsg_match_rows", d.id};
    std::vector<uint64_t> local_off((size_t)n_rows + 1);                  // the run's offsets, relative to its first byte
    for (uint32_t r = 0; r <= n_rows; ++r) local_off[r] = row_off[r0 + r] - byte0;
    // the sets this run's rows lie in, their first rows clamped to the run and counted from r0
    std::vector<uint32_t> set_first;
    uint32_t s0 = 0, n_sets = 0;
    if (many && many->n_sets) {
        const uint32_t *sf = many->set_first_row;
        s0 = (uint32_t)(std::upper_bound(sf + 1, sf + many->n_sets + 1, r0) - (sf + 1));       // the first set that ends behind r0
        const uint32_t s1 = (uint32_t)(std::lower_bound(sf, sf + many->n_sets, r1) - sf);      // the first set that begins at or behind r1
        n_sets = s1 - s0;
        set_first.resize((size_t)n_sets + 1);
        for (uint32_t i = 0; i <= n_sets; ++i) set_first[i] = std::min(std::max(sf[s0 + i], r0), r1) - r0;
    }
    d.calls.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    if (int32_t rc = ensure_lower_table(d)) return rc;
    trace.lap("offsets rebased, lock taken");
    const size_t n_words = ((size_t)n_rows + 63) / 64, n_planes = many ? many->n_queries : 1;
    Scratch scratch(d);                                                   // every early return below leaves through it: drained, then freed
    uint8_t *d_rows = nullptr, *d_cbytes = nullptr;
    uint64_t *d_off = nullptr, *d_ch = nullptr, *d_cfp = nullptr, *d_bits = nullptr;
    uint32_t *d_prog = nullptr, *d_fb = nullptr, *d_nfb = nullptr, *d_coff = nullptr, *d_ckind = nullptr, *d_rx = nullptr;
    uint32_t *d_poff = nullptr, *d_sfirst = nullptr;
    uint64_t *d_smask = nullptr;
    HIP_TRY(scratch.alloc(&d_rows, n_bytes + 64));
    HIP_TRY(scratch.alloc(&d_off, ((size_t)n_rows + 1) * 8));
    HIP_TRY(scratch.alloc(&d_ch, std::max<size_t>(n_conds, 1) * 2 * 32));
    HIP_TRY(scratch.alloc(&d_cfp, std::max<size_t>(n_conds, 1) * 2 * 8));
    HIP_TRY(scratch.alloc(&d_cbytes, (size_t)cond_len + 64));
    HIP_TRY(scratch.alloc(&d_coff, ((size_t)2 * n_conds + 1) * 4));
    HIP_TRY(scratch.alloc(&d_ckind, std::max<size_t>(n_conds, 1) * 4));
    HIP_TRY(scratch.alloc(&d_prog, std::max<size_t>(prog.size(), 1) * 4));
    HIP_TRY(scratch.alloc(&d_bits, n_words * n_planes * 8));
    HIP_TRY(scratch.alloc(&d_fb, (size_t)n_rows * 4));
    HIP_TRY(scratch.alloc(&d_nfb, 4));
    if (n_rx) HIP_TRY(scratch.alloc(&d_rx, rx_blob.size() * 4));
    if (many) HIP_TRY(scratch.alloc(&d_poff, many->prog_off.size() * 4));
    if (n_sets) {
        HIP_TRY(scratch.alloc(&d_sfirst, ((size_t)n_sets + 1) * 4));
        HIP_TRY(scratch.alloc(&d_smask, (size_t)n_sets * 8));
    }
    trace.lap("device buffers allocated");
    HIP_TRY(hipMemsetAsync(d_rows + n_bytes, 0, 64, d.stream));
    HIP_TRY(hipMemcpyAsync(d_off, local_off.data(), ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, d.stream));
    if (n_conds) {
        // the condition strings are hashed AND fingerprinted (under the context's secret key) on the device
        if (cond_len) HIP_TRY(hipMemcpyAsync(d_cbytes, cond_bytes, cond_len, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemsetAsync(d_cbytes + cond_len, 0, 64, d.stream));
        HIP_TRY(hipMemcpyAsync(d_coff, cond_off, ((size_t)2 * n_conds + 1) * 4, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d_ckind, cond_kinds, (size_t)n_conds * 4, hipMemcpyHostToDevice, d.stream));
        hipLaunchKernelGGL(bsg::k_hash_fp_entries, dim3((2 * n_conds + 255) / 256), dim3(256), 0, d.stream, (const uint8_t *)d_cbytes,
                           (const uint32_t *)d_coff, 2 * n_conds, d_ch, d_cfp, ctx->fp_key);
        HIP_TRY(hipGetLastError());
    }
    if (!prog.empty()) HIP_TRY(hipMemcpyAsync(d_prog, prog.data(), prog.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemsetAsync(d_nfb, 0, 4, d.stream));
    if (n_rx) HIP_TRY(hipMemcpyAsync(d_rx, rx_blob.data(), rx_blob.size() * 4, hipMemcpyHostToDevice, d.stream));
    if (many) HIP_TRY(hipMemcpyAsync(d_poff, many->prog_off.data(), many->prog_off.size() * 4, hipMemcpyHostToDevice, d.stream));
    if (n_sets) {
        HIP_TRY(hipMemcpyAsync(d_sfirst, set_first.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d_smask, many->set_mask + s0, (size_t)n_sets * 8, hipMemcpyHostToDevice, d.stream));
    }
    // The rows travel in chunks while the chunk before is being matched (RowUpload).  A surviving block is <= 10 MiB and goes in
    // one piece, in order on the one stream; a scan of many blocks in one call goes in pieces on the copy stream.
    RowUpload up(d, rows + byte0, d_rows, local_off.data(), n_rows, ctx->ingest_chunk_bytes);
    const uint32_t n_chunks = up.n_chunks();
    HIP_TRY(up.start(n_chunks > 1));
    trace.lap("small uploads enqueued");
    HIP_TRY(up.copy(0));
    EventList kev;                                                       // per chunk: kernel start, kernel stop
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t rf = up.cuts[c], re = up.cuts[c + 1];
        bsg::MatchArgs a{};
        a.rows = d_rows; a.row_off = d_off + rf; a.cond_h = d_ch; a.cond_fp = d_cfp; a.cond_kind = d_ckind; a.prog = d_prog; a.lower = d.d_lower;
        a.key = ctx->fp_key;
        a.out_bits = d_bits + rf / 64; a.fallback_rows = d_fb; a.n_fallback = d_nfb;
        a.n_rows = re - rf; a.row_base = rf; a.n_conds = n_conds; a.n_ops = (uint32_t)prog.size();
        HIP_TRY(kev.add(2));
        HIP_TRY(up.wait_landed(c));
        const hipEvent_t k0 = kev.v[(size_t)c * 2], k1 = kev.v[(size_t)c * 2 + 1];
        const dim3 grid((a.n_rows + bsg::kIngestThreads - 1) / bsg::kIngestThreads);
        if (many) {
            const bsg::MatchManyArgs m{d_poff, d_sfirst, d_smask, n_words, many->n_queries, n_sets};
            const bsg::RxArgs x{d_rx, (uint32_t)rx_blob.size(), n_rx};
            const uint32_t rx_lds = bsg::kMatchManyLdsBytes + (uint32_t)rx_blob.size() * 4;
            if (n_rx && tok)
                hipExtLaunchKernelGGL(bsg::k_match_rows_many_regex_tok, grid, dim3(bsg::kIngestThreads), rx_lds, d.stream, k0, k1, 0, a, x, m, *tok);
            else if (n_rx)
                hipExtLaunchKernelGGL(bsg::k_match_rows_many_regex, grid, dim3(bsg::kIngestThreads), rx_lds, d.stream, k0, k1, 0, a, x, m);
            else if (tok)
                hipExtLaunchKernelGGL(bsg::k_match_rows_many_tok, grid, dim3(bsg::kIngestThreads), bsg::kMatchManyLdsBytes, d.stream, k0, k1, 0, a, m, *tok);
            else
                hipExtLaunchKernelGGL(bsg::k_match_rows_many, grid, dim3(bsg::kIngestThreads), bsg::kMatchManyLdsBytes, d.stream, k0, k1, 0, a, m);
        } else if (n_rx && tok) {
            const bsg::RxArgs x{d_rx, (uint32_t)rx_blob.size(), n_rx};
            hipExtLaunchKernelGGL(bsg::k_match_rows_regex_tok, grid, dim3(bsg::kIngestThreads), bsg::kMatchLdsBytes + (uint32_t)rx_blob.size() * 4,
                                  d.stream, k0, k1, 0, a, x, *tok);
        } else if (n_rx) {
            const bsg::RxArgs x{d_rx, (uint32_t)rx_blob.size(), n_rx};
            hipExtLaunchKernelGGL(bsg::k_match_rows_regex, grid, dim3(bsg::kIngestThreads), bsg::kMatchLdsBytes + (uint32_t)rx_blob.size() * 4,
                                  d.stream, k0, k1, 0, a, x);
        } else if (tok) {
            hipExtLaunchKernelGGL(bsg::k_match_rows_tok, grid, dim3(bsg::kIngestThreads), bsg::kMatchLdsBytes, d.stream, k0, k1, 0, a, *tok);
        } else {
            hipExtLaunchKernelGGL(bsg::k_match_rows, grid, dim3(bsg::kIngestThreads), bsg::kMatchLdsBytes, d.stream, k0, k1, 0, a);
        }
        HIP_TRY(hipGetLastError());
        if (c + 1 < n_chunks) HIP_TRY(up.copy(c + 1));                   // K(c) is running: now the next chunk's bytes
    }
    trace.lap("all chunks enqueued");
    uint32_t nfb = 0;
    if (!many || many->call_words == n_words)
        HIP_TRY(hipMemcpyAsync(out_bits + r0 / 64, d_bits, n_words * n_planes * 8, hipMemcpyDeviceToHost, d.stream));
    else                                                                 // this run's words of every plane
        HIP_TRY(hipMemcpy2DAsync(out_bits + r0 / 64, many->call_words * 8, d_bits, n_words * 8, n_words * 8, n_planes, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipMemcpyAsync(&nfb, d_nfb, 4, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    trace.lap("matched, bits back");
    *ms = 0.f;
    for (uint32_t c = 0; c < n_chunks; ++c) { float t = 0.f; (void)hipEventElapsedTime(&t, kev.v[(size_t)c * 2], kev.v[(size_t)c * 2 + 1]); *ms += t; }
    fb.resize(nfb);
    if (nfb) HIP_TRY(hipMemcpy(fb.data(), d_fb, (size_t)nfb * 4, hipMemcpyDeviceToHost));
    for (uint32_t &r : fb) r += r0;
    scratch.done();                        // every kernel has finished, and each waited for its chunk's copy
    return BSG_OK;
}

// What every row-matcher call checks of its rows and conditions (the kinds themselves are the caller's); cond_len / n_bytes out.
int32_t check_match_inputs(const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows, const uint8_t *cond_bytes, const uint32_t *cond_off,
                           const uint32_t *cond_kinds, uint32_t n_conds, const uint64_t *out_bits, const uint32_t *out_n_fallback,
                           uint32_t &cond_len, uint64_t &n_bytes)
{
    if (!out_n_fallback || (n_rows && (!row_off || !out_bits))) return fail(BSG_E_INVALID, "null argument");
    if (n_conds && (!cond_off || !cond_kinds)) return fail(BSG_E_INVALID, "conditions are null");
    if (n_conds > bsg::kMatchMaxConds) return fail(BSG_E_UNSUPPORTED, "%u conditions (the device matcher holds %u)", n_conds, bsg::kMatchMaxConds);
    for (uint32_t e = 0; e < 2 * n_conds; ++e)
        if (cond_off[e + 1] < cond_off[e]) return fail(BSG_E_INVALID, "cond_off not monotone at %u", e);
    cond_len = n_conds ? cond_off[2 * n_conds] : 0;
    if (cond_len && !cond_bytes) return fail(BSG_E_INVALID, "cond_bytes is null");
    for (uint32_t r = 0; r < n_rows; ++r)
        if (row_off[r + 1] < row_off[r]) return fail(BSG_E_INVALID, "row_off not monotone at %u", r);
    n_bytes = n_rows ? row_off[n_rows] - row_off[0] : 0;
    if (n_bytes && !rows) return fail(BSG_E_INVALID, "rows is null");
    return BSG_OK;
}

// The validated, lowered call on the context's devices.
// Surviving blocks are independent (query_exec.go:729-764): a large scan is cut into one contiguous run of rows per
// device (on 64-row boundaries: whole words of out_bits, about equal bytes); a small one takes one device.
int32_t match_rows_run(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows, uint64_t n_bytes,
                       const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds, uint32_t cond_len,
                       const std::vector<uint32_t> &prog, const std::vector<uint32_t> &rx_blob, uint32_t n_rx, const bsg::TokSpec *tok,
                       uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback, const ManyPlan *many = nullptr)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    uint32_t want = (nd > 1 && n_bytes >= ctx->shard_min_row_bytes) ? nd : 1;
    std::vector<uint32_t> cuts{0};
    for (uint32_t i = 1; i < want; ++i) {
        const uint64_t target = row_off[0] + n_bytes * i / want;
        uint32_t r = (uint32_t)(std::lower_bound(row_off, row_off + n_rows, target) - row_off);
        r = r / 64 * 64;
        if (r > cuts.back() && r < n_rows) cuts.push_back(r);
    }
    cuts.push_back(n_rows);
    const uint32_t n_parts = (uint32_t)cuts.size() - 1;
    std::vector<std::vector<uint32_t>> fbs(n_parts);
    std::vector<float> ms(n_parts, 0.f);
    const uint32_t first = n_parts == 1 ? pick_device(ctx) : 0;
    if (int32_t rc = run_parts(n_parts, [&](uint32_t i) -> int32_t {
            return match_rows_on(ctx, *ctx->devs[(first + i) % nd], rows, row_off, cuts[i], cuts[i + 1], cond_bytes, cond_off, cond_kinds, n_conds,
                                 cond_len, prog, rx_blob, n_rx, tok, out_bits, fbs[i], &ms[i], many);
        })) return rc;
    std::vector<uint32_t> fb;
    for (auto &v : fbs) fb.insert(fb.end(), v.begin(), v.end());
    std::sort(fb.begin(), fb.end());
    *out_n_fallback = (uint32_t)fb.size();
    if (!fb.empty() && out_fallback_rows) memcpy(out_fallback_rows, fb.data(), (size_t)std::min<uint32_t>((uint32_t)fb.size(), fallback_cap) * 4);
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        ctx->last_match_ms = *std::max_element(ms.begin(), ms.end());
    }
    if (fb.size() > fallback_cap && out_fallback_rows)
        return fail(BSG_E_INVALID, "%zu rows need the host matcher, caller's list holds %u", fb.size(), fallback_cap);
    return BSG_OK;
}

// bsg_match_rows (max_kind 2), bsg_match_rows_regex (max_kind 3) and bsg_match_rows_tok (max_kind 3, a spec; NULL = default)
int32_t match_rows_call(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                        const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                        const uint32_t *prog_ops, uint32_t n_ops,
                        uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback, uint32_t max_kind,
                        const bsg_tokenizer *tok_in = nullptr)
{
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    bsg_tokenizer rec{};
    bsg::TokSpec spec{};
    bool is_default = true;
    if (int32_t rc = tok_spec(tok_in, rec, spec, is_default)) return rc;
    const bsg::TokSpec *tok = is_default ? nullptr : &spec;
    if (n_ops && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    uint32_t cond_len = 0;
    uint64_t n_bytes = 0;
    if (int32_t rc = check_match_inputs(rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_n_fallback, cond_len, n_bytes))
        return rc;
    for (uint32_t c = 0; c < n_conds; ++c)
        if (cond_kinds[c] > max_kind) return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, cond_kinds[c]);
    std::vector<uint32_t> ident(n_conds), prog;
    for (uint32_t c = 0; c < n_conds; ++c) ident[c] = c;
    uint32_t depth = 1;
    if (int32_t rc = lower_program(prog_ops, n_ops, n_conds, ident, prog, depth)) return rc;
    if (depth > 64 || prog.size() > bsg::kMatchMaxOps)
        return fail(BSG_E_UNSUPPORTED, "expression too large for the device matcher (depth %u, %zu ops)", depth, prog.size());
    std::vector<uint32_t> rx_blob;
    uint32_t n_rx = 0;
    if (int32_t rc = build_rx_blob(cond_bytes, cond_off, cond_kinds, n_conds, rx_blob, n_rx)) return rc;
    *out_n_fallback = 0;
    if (n_rows == 0) return BSG_OK;
    return match_rows_run(ctx, rows, row_off, n_rows, n_bytes, cond_bytes, cond_off, cond_kinds, n_conds, cond_len, prog, rx_blob, n_rx, tok, out_bits,
                          out_fallback_rows, fallback_cap, out_n_fallback);
}

// bsg_match_rows_many (max_kind 2) and bsg_match_rows_many_regex (max_kind 3): n_queries programs over one table of distinct
// conditions, one upload and one walk of the rows
int32_t match_rows_many_call(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                             const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                             const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                             const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok_in,
                             uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback,
                             uint32_t max_kind)
{
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    bsg_tokenizer rec{};
    bsg::TokSpec spec{};
    bool is_default = true;
    if (int32_t rc = tok_spec(tok_in, rec, spec, is_default)) return rc;
    const bsg::TokSpec *tok = is_default ? nullptr : &spec;
    if (n_queries > bsg::kMatchManyMaxQueries)
        return fail(BSG_E_UNSUPPORTED, "%u queries (one batched match call holds %u)", n_queries, bsg::kMatchManyMaxQueries);
    if (n_queries && !prog_off) return fail(BSG_E_INVALID, "prog_off is null");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
    if (n_queries && prog_off[n_queries] > prog_off[0] && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    uint32_t cond_len = 0;
    uint64_t n_bytes = 0;
    if (int32_t rc = check_match_inputs(rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_n_fallback, cond_len, n_bytes))
        return rc;
    for (uint32_t c = 0; c < n_conds; ++c) {
        if (cond_kinds[c] == BSG_KIND_FIELD_REGEX && max_kind < BSG_KIND_FIELD_REGEX)
            return fail(BSG_E_UNSUPPORTED, "condition %u: FieldRegex conditions are not matched by the batched call (use bsg_match_rows_regex)", c);
        if (cond_kinds[c] > max_kind) return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, cond_kinds[c]);
    }
    if (n_sets) {
        if (!set_first_row || !query_mask_of_set) return fail(BSG_E_INVALID, "set table is null");
        if (set_first_row[0] != 0 || set_first_row[n_sets] != n_rows)
            return fail(BSG_E_INVALID, "set_first_row spans rows [%u, %u), the call has %u", set_first_row[0], set_first_row[n_sets], n_rows);
        for (uint32_t s = 0; s < n_sets; ++s) {
            if (set_first_row[s + 1] < set_first_row[s]) return fail(BSG_E_INVALID, "set_first_row not monotone at %u", s);
            if (n_queries < 64 && (query_mask_of_set[s] >> n_queries) != 0)
                return fail(BSG_E_INVALID, "set %u: mask 0x%llx has bits at or above query %u", s, (unsigned long long)query_mask_of_set[s], n_queries);
        }
    }
    ManyPlan plan{{0}, set_first_row, query_mask_of_set, n_sets, n_queries, ((size_t)n_rows + 63) / 64};
    std::vector<uint32_t> ident(n_conds), prog, one;
    for (uint32_t c = 0; c < n_conds; ++c) ident[c] = c;
    for (uint32_t q = 0; q < n_queries; ++q) {
        uint32_t depth = 1;
        if (int32_t rc = lower_program(prog_ops + prog_off[q], prog_off[q + 1] - prog_off[q], n_conds, ident, one, depth)) return rc;
        if (depth > 64) return fail(BSG_E_UNSUPPORTED, "query %u: expression too deep for the device matcher (depth %u)", q, depth);
        prog.insert(prog.end(), one.begin(), one.end());
        if (prog.size() > bsg::kMatchManyMaxOps)
            return fail(BSG_E_UNSUPPORTED, "the batch's programs hold more than %u lowered ops (at query %u)", bsg::kMatchManyMaxOps, q);
        plan.prog_off.push_back((uint32_t)prog.size());
    }
    // the regex conditions' tables, each with the queries that use it (a table without any: exactly bsg_match_rows_many's kernels)
    std::vector<uint32_t> rx_blob;
    uint32_t n_rx = 0;
    if (max_kind >= BSG_KIND_FIELD_REGEX && n_queries) {
        const std::vector<uint64_t> users = bsh_rxg::user_masks(prog_ops, prog_off, n_queries, n_conds);
        if (int32_t rc = build_rx_blob(cond_bytes, cond_off, cond_kinds, n_conds, rx_blob, n_rx, bsg::kRxManyLdsCap, users.data())) return rc;
    }
    if (n_queries == 0 || n_rows == 0) return BSG_OK;
    *out_n_fallback = 0;
    return match_rows_run(ctx, rows, row_off, n_rows, n_bytes, cond_bytes, cond_off, cond_kinds, n_conds, cond_len, prog, rx_blob, n_rx, tok, out_bits,
                          out_fallback_rows, fallback_cap, out_n_fallback, &plan);
}

// ---- bsg_match_rows_wide: any number of queries over one condition table (k_match_rows_store*, then k_eval_row_programs) ----
static_assert(bsh_wide::kWideLdsCap == bsg::kRxWideLdsCap && sizeof(bsh_wide::EvalItem) == sizeof(bsg::RowEvalItem) &&
                  offsetof(bsh_wide::EvalItem, stride) == offsetof(bsg::RowEvalItem, stride),
              "host/wide_plan.hpp states the kernels' limits and item layout");

// what a part needs of the validated call (sets always materialised: the implicit set is one set with every query)
struct WidePlan {
    const uint32_t *set_first_row, *set_query_off, *set_queries;
    uint32_t n_sets, n_queries;
    std::vector<uint32_t> prog_off;            // [n_queries + 1] into the lowered programs
    std::vector<uint64_t> set_cond_mask;       // [n_sets]
    std::vector<uint64_t> set_word0;           // [n_sets + 1]: the first result word of the set's first pair
};

// rows [r0, r1) (r0 a set-relative multiple of 64) on one device: the storing walk chunk by chunk, then one evaluation launch over
// the part's items.  direct: the part is the whole call and its words go straight to out_bits; else they are scattered on the host
// into the call's layout (a set cut by a part boundary has some of its tiles here and some on the next device).
int32_t match_rows_wide_on(bsg_ctx *ctx, Device &d, const uint8_t *rows, const uint64_t *row_off, uint32_t r0, uint32_t r1,
                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds, uint32_t cond_len,
                           const std::vector<uint32_t> &prog, const std::vector<uint32_t> &rx_blob, uint32_t n_rx, const bsg::TokSpec *tok,
                           const WidePlan &wp, bool direct, uint64_t *out_bits, std::vector<uint32_t> &fb, float *ms)
{
    const uint32_t n_rows = r1 - r0;
    const uint64_t byte0 = row_off[r0], n_bytes = row_off[r1] - byte0;
    const LabTrace trace{"bsg_match_rows_wide", d.id};
    std::vector<uint64_t> local_off((size_t)n_rows + 1);
    for (uint32_t r = 0; r <= n_rows; ++r) local_off[r] = row_off[r0 + r] - byte0;
    const bsh_wide::PartSets ps = bsh_wide::part_sets(wp.set_first_row, wp.set_query_off, wp.n_sets, r0, r1);
    const uint32_t n_sets = ps.n(), pair0 = ps.pair_off[0], n_pairs = ps.pair_off[n_sets] - pair0;
    std::vector<uint32_t> pair_off_local(ps.pair_off);
    for (uint32_t &v : pair_off_local) v -= pair0;
    std::vector<bsh_wide::EvalItem> items;
    uint64_t part_words = 0;
    if (!bsh_wide::eval_items(ps, items, part_words))
        return fail(BSG_E_UNSUPPORTED, "more than %u (tile, pair range) items on one device", bsh_wide::kMaxItems);
    d.calls.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    if (int32_t rc = ensure_lower_table(d)) return rc;
    trace.lap("part planned, lock taken");
    Scratch scratch(d);
    uint8_t *d_rows = nullptr, *d_cbytes = nullptr, *d_state = nullptr;
    uint64_t *d_off = nullptr, *d_ch = nullptr, *d_cfp = nullptr, *d_sat = nullptr, *d_out = nullptr, *d_smask = nullptr;
    uint32_t *d_prog = nullptr, *d_fb = nullptr, *d_nfb = nullptr, *d_coff = nullptr, *d_ckind = nullptr, *d_rx = nullptr;
    uint32_t *d_poff = nullptr, *d_sfirst = nullptr, *d_spair = nullptr, *d_pairs = nullptr;
    bsg::RowEvalItem *d_items = nullptr;
    HIP_TRY(scratch.alloc(&d_rows, n_bytes + 64));
    HIP_TRY(scratch.alloc(&d_off, ((size_t)n_rows + 1) * 8));
    HIP_TRY(scratch.alloc(&d_ch, std::max<size_t>(n_conds, 1) * 2 * 32));
    HIP_TRY(scratch.alloc(&d_cfp, std::max<size_t>(n_conds, 1) * 2 * 8));
    HIP_TRY(scratch.alloc(&d_cbytes, (size_t)cond_len + 64));
    HIP_TRY(scratch.alloc(&d_coff, ((size_t)2 * n_conds + 1) * 4));
    HIP_TRY(scratch.alloc(&d_ckind, std::max<size_t>(n_conds, 1) * 4));
    HIP_TRY(scratch.alloc(&d_prog, std::max<size_t>(prog.size(), 1) * 4));
    HIP_TRY(scratch.alloc(&d_poff, wp.prog_off.size() * 4));
    HIP_TRY(scratch.alloc(&d_sat, (size_t)n_rows * 8));
    HIP_TRY(scratch.alloc(&d_state, (size_t)n_rows));
    HIP_TRY(scratch.alloc(&d_out, std::max<uint64_t>(part_words, 1) * 8));
    HIP_TRY(scratch.alloc(&d_fb, (size_t)n_rows * 4));
    HIP_TRY(scratch.alloc(&d_nfb, 4));
    HIP_TRY(scratch.alloc(&d_sfirst, ((size_t)n_sets + 1) * 4));
    HIP_TRY(scratch.alloc(&d_spair, ((size_t)n_sets + 1) * 4));
    HIP_TRY(scratch.alloc(&d_smask, (size_t)n_sets * 8));
    HIP_TRY(scratch.alloc(&d_pairs, std::max<size_t>(n_pairs, 1) * 4));
    HIP_TRY(scratch.alloc(&d_items, std::max<size_t>(items.size(), 1) * sizeof(bsg::RowEvalItem)));
    if (n_rx) HIP_TRY(scratch.alloc(&d_rx, rx_blob.size() * 4));
    trace.lap("device buffers allocated");
    HIP_TRY(hipMemsetAsync(d_rows + n_bytes, 0, 64, d.stream));
    HIP_TRY(hipMemcpyAsync(d_off, local_off.data(), ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, d.stream));
    if (n_conds) {
        if (cond_len) HIP_TRY(hipMemcpyAsync(d_cbytes, cond_bytes, cond_len, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemsetAsync(d_cbytes + cond_len, 0, 64, d.stream));
        HIP_TRY(hipMemcpyAsync(d_coff, cond_off, ((size_t)2 * n_conds + 1) * 4, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d_ckind, cond_kinds, (size_t)n_conds * 4, hipMemcpyHostToDevice, d.stream));
        hipLaunchKernelGGL(bsg::k_hash_fp_entries, dim3((2 * n_conds + 255) / 256), dim3(256), 0, d.stream, (const uint8_t *)d_cbytes,
                           (const uint32_t *)d_coff, 2 * n_conds, d_ch, d_cfp, ctx->fp_key);
        HIP_TRY(hipGetLastError());
    }
    if (!prog.empty()) HIP_TRY(hipMemcpyAsync(d_prog, prog.data(), prog.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d_poff, wp.prog_off.data(), wp.prog_off.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemsetAsync(d_nfb, 0, 4, d.stream));
    if (n_rx) HIP_TRY(hipMemcpyAsync(d_rx, rx_blob.data(), rx_blob.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d_sfirst, ps.first_row.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d_spair, pair_off_local.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d_smask, wp.set_cond_mask.data() + ps.s0, (size_t)n_sets * 8, hipMemcpyHostToDevice, d.stream));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(d_pairs, wp.set_queries + pair0, (size_t)n_pairs * 4, hipMemcpyHostToDevice, d.stream));
    if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::RowEvalItem), hipMemcpyHostToDevice, d.stream));
    RowUpload up(d, rows + byte0, d_rows, local_off.data(), n_rows, ctx->ingest_chunk_bytes);
    const uint32_t n_chunks = up.n_chunks();
    HIP_TRY(up.start(n_chunks > 1));
    trace.lap("small uploads enqueued");
    HIP_TRY(up.copy(0));
    EventList kev;                                                       // per chunk: walk start, walk stop; then the evaluation's two
    const bsg::RxArgs x{d_rx, (uint32_t)rx_blob.size(), n_rx};
    const uint32_t lds = bsg::kMatchWideLdsBytes + (uint32_t)rx_blob.size() * 4;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t rf = up.cuts[c], re = up.cuts[c + 1];
        bsg::MatchArgs a{};
        a.rows = d_rows; a.row_off = d_off + rf; a.cond_h = d_ch; a.cond_fp = d_cfp; a.cond_kind = d_ckind; a.lower = d.d_lower;
        a.key = ctx->fp_key;
        a.fallback_rows = d_fb; a.n_fallback = d_nfb;
        a.n_rows = re - rf; a.row_base = rf; a.n_conds = n_conds;
        const bsg::MatchWideArgs wd{d_sfirst, d_smask, d_spair, d_sat + rf, d_state + rf, n_sets};
        HIP_TRY(kev.add(2));
        HIP_TRY(up.wait_landed(c));
        const hipEvent_t k0 = kev.v[(size_t)c * 2], k1 = kev.v[(size_t)c * 2 + 1];
        const dim3 grid((a.n_rows + bsg::kIngestThreads - 1) / bsg::kIngestThreads);
        if (n_rx && tok) hipExtLaunchKernelGGL(bsg::k_match_rows_store_regex_tok, grid, dim3(bsg::kIngestThreads), lds, d.stream, k0, k1, 0, a, x, wd, *tok);
        else if (n_rx) hipExtLaunchKernelGGL(bsg::k_match_rows_store_regex, grid, dim3(bsg::kIngestThreads), lds, d.stream, k0, k1, 0, a, x, wd);
        else if (tok) hipExtLaunchKernelGGL(bsg::k_match_rows_store_tok, grid, dim3(bsg::kIngestThreads), lds, d.stream, k0, k1, 0, a, wd, *tok);
        else hipExtLaunchKernelGGL(bsg::k_match_rows_store, grid, dim3(bsg::kIngestThreads), lds, d.stream, k0, k1, 0, a, wd);
        HIP_TRY(hipGetLastError());
        if (c + 1 < n_chunks) HIP_TRY(up.copy(c + 1));
    }
    trace.lap("all chunks enqueued");
    HIP_TRY(kev.add(2));
    if (!items.empty()) {
        const bsg::RowEvalArgs e{d_items, d_pairs, d_poff, d_prog, d_sat, d_state, d_out, (uint32_t)items.size()};
        const uint32_t per_block = bsg::kRowEvalThreads / 64;
        hipExtLaunchKernelGGL(bsg::k_eval_row_programs, dim3(((uint32_t)items.size() + per_block - 1) / per_block), dim3(bsg::kRowEvalThreads), 0, d.stream,
                              kev.v[(size_t)n_chunks * 2], kev.v[(size_t)n_chunks * 2 + 1], 0, e);
        HIP_TRY(hipGetLastError());
    }
    uint32_t nfb = 0;
    std::vector<uint64_t> staged;
    if (part_words) {
        uint64_t *dst = out_bits + wp.set_word0[ps.s0];
        if (!direct) { staged.resize(part_words); dst = staged.data(); }
        HIP_TRY(hipMemcpyAsync(dst, d_out, part_words * 8, hipMemcpyDeviceToHost, d.stream));
    }
    HIP_TRY(hipMemcpyAsync(&nfb, d_nfb, 4, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    trace.lap("matched, words back");
    *ms = 0.f;
    for (uint32_t c = 0; c < n_chunks + (items.empty() ? 0u : 1u); ++c) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, kev.v[(size_t)c * 2], kev.v[(size_t)c * 2 + 1]);
        *ms += t;
    }
    fb.resize(nfb);
    if (nfb) HIP_TRY(hipMemcpy(fb.data(), d_fb, (size_t)nfb * 4, hipMemcpyDeviceToHost));
    for (uint32_t &r : fb) r += r0;
    scratch.done();
    if (!direct) {                                                       // the part's layout -> the call's: per pair, the part's tiles of the set
        uint64_t at = 0;
        for (uint32_t ls = 0; ls < n_sets; ++ls) {
            const uint32_t s = ps.s0 + ls, tiles = bsh_wide::tiles_of(ps.first_row[ls + 1] - ps.first_row[ls]);
            const uint32_t set_tiles = bsh_wide::tiles_of(wp.set_first_row[s + 1] - wp.set_first_row[s]);
            for (uint32_t p = ps.pair_off[ls]; p < ps.pair_off[ls + 1] && tiles; ++p, at += tiles)
                memcpy(out_bits + wp.set_word0[s] + (uint64_t)(p - wp.set_query_off[s]) * set_tiles + ps.tile0[ls], staged.data() + at, (size_t)tiles * 8);
        }
    }
    return BSG_OK;
}

int32_t wide_size_status(bsh_wide::SizeStatus st, uint32_t bad_set, const uint32_t *set_first_row, uint32_t n_sets, uint32_t n_rows)
{
    switch (st) {
    case bsh_wide::SizeStatus::Ok: return BSG_OK;
    case bsh_wide::SizeStatus::Null: return fail(BSG_E_INVALID, "set table is null (or given without its number of sets)");
    case bsh_wide::SizeStatus::SetSpan:
        return fail(BSG_E_INVALID, "set_first_row spans rows [%u, %u), the call has %u", set_first_row[0], set_first_row[n_sets], n_rows);
    case bsh_wide::SizeStatus::SetOrder: return fail(BSG_E_INVALID, "set_first_row not monotone at %u", bad_set);
    default: return fail(BSG_E_INVALID, "set_query_off not monotone (or not beginning at 0) at %u", bad_set);
    }
}

int32_t match_rows_wide_call(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                             const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                             const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                             const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                             const bsg_tokenizer *tok_in, uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                             uint32_t *out_n_fallback)
{
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    bsg_tokenizer rec{};
    bsg::TokSpec spec{};
    bool is_default = true;
    if (int32_t rc = tok_spec(tok_in, rec, spec, is_default)) return rc;
    const bsg::TokSpec *tok = is_default ? nullptr : &spec;
    if (n_queries > bsh_wide::kMaxQueries)
        return fail(BSG_E_UNSUPPORTED, "%u queries (one wide match call holds %u)", n_queries, bsh_wide::kMaxQueries);
    if (n_queries && !prog_off) return fail(BSG_E_INVALID, "prog_off is null");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
    if (n_queries && prog_off[n_queries] > prog_off[0] && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    uint32_t cond_len = 0;
    uint64_t n_bytes = 0;
    if (int32_t rc = check_match_inputs(rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_n_fallback, cond_len, n_bytes))
        return rc;
    for (uint32_t c = 0; c < n_conds; ++c)
        if (cond_kinds[c] > BSG_KIND_FIELD_REGEX) return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, cond_kinds[c]);
    // the sets: the caller's, or one implicit set of all rows with every query
    WidePlan wp{set_first_row, set_query_off, set_queries, n_sets, n_queries, {0}, {}, {}};
    std::vector<uint32_t> implicit_first, implicit_off, implicit_queries;
    if (n_sets == 0) {
        if (set_first_row || set_query_off || set_queries) return fail(BSG_E_INVALID, "a set table without its number of sets");
        implicit_first = {0, n_rows};
        implicit_off = {0, n_queries};
        implicit_queries.resize(n_queries);
        for (uint32_t q = 0; q < n_queries; ++q) implicit_queries[q] = q;
        wp.set_first_row = implicit_first.data(); wp.set_query_off = implicit_off.data(); wp.set_queries = implicit_queries.data(); wp.n_sets = 1;
    } else {
        uint32_t bad = 0;
        const bsh_wide::SizeStatus st = bsh_wide::pair_words(set_first_row, set_query_off, n_sets, n_rows, n_queries, nullptr, nullptr, &bad);
        if (int32_t rc = wide_size_status(st, bad, set_first_row, n_sets, n_rows)) return rc;
        if (set_query_off[n_sets] > bsh_wide::kMaxPairs)
            return fail(BSG_E_UNSUPPORTED, "%u (set, query) pairs (one wide match call holds %u)", set_query_off[n_sets], bsh_wide::kMaxPairs);
        if (set_query_off[n_sets] && !set_queries) return fail(BSG_E_INVALID, "set_queries is null");
        for (uint32_t s = 0; s < n_sets; ++s)
            for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) {
                if (set_queries[p] >= n_queries) return fail(BSG_E_INVALID, "set %u lists query %u of %u", s, set_queries[p], n_queries);
                if (p > set_query_off[s] && set_queries[p] <= set_queries[p - 1])
                    return fail(BSG_E_INVALID, "set %u: its query list is not strictly ascending at pair %u", s, p);
            }
    }
    std::vector<uint32_t> ident(n_conds), prog, one;
    for (uint32_t c = 0; c < n_conds; ++c) ident[c] = c;
    for (uint32_t q = 0; q < n_queries; ++q) {
        uint32_t depth = 1;
        if (int32_t rc = lower_program(prog_ops + prog_off[q], prog_off[q + 1] - prog_off[q], n_conds, ident, one, depth)) return rc;
        if (depth > 64) return fail(BSG_E_UNSUPPORTED, "query %u: expression too deep for the device matcher (depth %u)", q, depth);
        prog.insert(prog.end(), one.begin(), one.end());
        if (prog.size() > bsh_wide::kMaxOps)
            return fail(BSG_E_UNSUPPORTED, "the call's programs hold more than %u lowered ops (at query %u)", bsh_wide::kMaxOps, q);
        wp.prog_off.push_back((uint32_t)prog.size());
    }
    std::vector<uint32_t> rx_blob;
    uint32_t n_rx = 0;
    if (int32_t rc = build_rx_blob(cond_bytes, cond_off, cond_kinds, n_conds, rx_blob, n_rx, bsg::kRxWideLdsCap)) return rc;
    const uint32_t n_pairs = wp.set_query_off[wp.n_sets];
    if (n_rows == 0 || n_pairs == 0) return BSG_OK;
    wp.set_cond_mask = bsh_wide::set_cond_masks(bsh_wide::query_cond_masks(prog_ops, prog_off, n_queries, n_conds), wp.set_query_off, wp.set_queries, wp.n_sets);
    wp.set_word0.assign((size_t)wp.n_sets + 1, 0);
    for (uint32_t s = 0; s < wp.n_sets; ++s)
        wp.set_word0[s + 1] = wp.set_word0[s] + (uint64_t)bsh_wide::tiles_of(wp.set_first_row[s + 1] - wp.set_first_row[s]) *
                                                    (wp.set_query_off[s + 1] - wp.set_query_off[s]);
    *out_n_fallback = 0;
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const uint32_t want = (nd > 1 && n_bytes >= ctx->shard_min_row_bytes) ? nd : 1;
    const std::vector<uint32_t> cuts = bsh_wide::part_cuts(row_off, n_rows, wp.set_first_row, wp.n_sets, want);
    const uint32_t n_parts = (uint32_t)cuts.size() - 1;
    std::vector<std::vector<uint32_t>> fbs(n_parts);
    std::vector<float> ms(n_parts, 0.f);
    const uint32_t first = n_parts == 1 ? pick_device(ctx) : 0;
    if (int32_t rc = run_parts(n_parts, [&](uint32_t i) -> int32_t {
            return match_rows_wide_on(ctx, *ctx->devs[(first + i) % nd], rows, row_off, cuts[i], cuts[i + 1], cond_bytes, cond_off, cond_kinds, n_conds,
                                      cond_len, prog, rx_blob, n_rx, tok, wp, n_parts == 1, out_bits, fbs[i], &ms[i]);
        })) return rc;
    std::vector<uint32_t> fb;
    for (auto &v : fbs) fb.insert(fb.end(), v.begin(), v.end());
    std::sort(fb.begin(), fb.end());
    *out_n_fallback = (uint32_t)fb.size();
    if (!fb.empty() && out_fallback_rows) memcpy(out_fallback_rows, fb.data(), (size_t)std::min<uint32_t>((uint32_t)fb.size(), fallback_cap) * 4);
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        ctx->last_match_ms = *std::max_element(ms.begin(), ms.end());
    }
    if (fb.size() > fallback_cap && out_fallback_rows)
        return fail(BSG_E_INVALID, "%zu rows need the host matcher, caller's list holds %u", fb.size(), fallback_cap);
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_match_rows_wide(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                            const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                            const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                            const bsg_tokenizer *tok,
                            uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_wide_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, prog_off, n_queries, set_first_row,
                                set_query_off, set_queries, n_sets, tok, out_bits, out_fallback_rows, fallback_cap, out_n_fallback);
}

int32_t bsg_match_wide_size(const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets, uint32_t n_rows, uint32_t n_queries,
                            uint64_t *out_pair_word_off, uint64_t *out_total_words)
{
    if (!out_total_words) return fail(BSG_E_INVALID, "out_total_words is null");
    uint32_t bad = 0;
    const bsh_wide::SizeStatus st = bsh_wide::pair_words(set_first_row, set_query_off, n_sets, n_rows, n_queries, out_pair_word_off, out_total_words, &bad);
    return wide_size_status(st, bad, set_first_row, n_sets, n_rows);
}

int32_t bsg_match_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                       const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                       const uint32_t *prog_ops, uint32_t n_ops,
                       uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, n_ops, out_bits, out_fallback_rows,
                           fallback_cap, out_n_fallback, BSG_KIND_FIELD_TOKEN);
}

int32_t bsg_match_rows_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                             const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                             const uint32_t *prog_ops, uint32_t n_ops,
                             uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, n_ops, out_bits, out_fallback_rows,
                           fallback_cap, out_n_fallback, BSG_KIND_FIELD_REGEX);
}

int32_t bsg_match_rows_tok(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                           const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                           uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, n_ops, out_bits, out_fallback_rows,
                           fallback_cap, out_n_fallback, BSG_KIND_FIELD_REGEX, tok);
}

int32_t bsg_match_rows_many(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                            const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                            const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                            uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_many_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, prog_off, n_queries, set_first_row,
                                query_mask_of_set, n_sets, tok, out_bits, out_fallback_rows, fallback_cap, out_n_fallback, BSG_KIND_FIELD_TOKEN);
}

int32_t bsg_match_rows_many_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                  const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                  const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                  const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                  uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    return match_rows_many_call(ctx, rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, prog_ops, prog_off, n_queries, set_first_row,
                                query_mask_of_set, n_sets, tok, out_bits, out_fallback_rows, fallback_cap, out_n_fallback, BSG_KIND_FIELD_REGEX);
}

int32_t bsg_pinned_alloc(bsg_ctx *ctx, uint64_t n_bytes, void **out_ptr)
{
    BSG_ENTER(ctx);
    if (!ctx || !out_ptr) return fail(BSG_E_INVALID, "null argument");
    Device &d = *ctx->devs[0];
    if (int32_t rc = use_device(d)) return rc;
    void *p = nullptr;
    // portable: the rows / bitsets a caller keeps here are copied to and from EVERY device of the context (the parts of one
    // call run on different devices), not only the one that is current now
    const hipError_t e = hipHostMalloc(&p, std::max<uint64_t>(n_bytes, 1), hipHostMallocPortable);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? BSG_E_NOMEM : BSG_E_HIP, "hipHostMalloc: %s", hipGetErrorString(e));
    *out_ptr = p;
    return BSG_OK;
}

int32_t bsg_pinned_free(bsg_ctx *ctx, void *ptr)
{
    BSG_ENTER(ctx);
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    if (!ptr) return BSG_OK;
    HIP_TRY(hipHostFree(ptr));
    return BSG_OK;
}

// Page-lock memory the caller already owns (C memory, an mmap of a file or of shared memory — never Go-heap memory): copies
// to and from it become plain DMA.  One-process-per-GPU layers register slices of ONE shared-memory segment so every
// rank's survivors land where the gathering rank reads them (a host-side gather without a collective).
int32_t bsg_host_register(bsg_ctx *ctx, void *ptr, uint64_t n_bytes)
{
    BSG_ENTER(ctx);
    if (!ptr || !n_bytes) return fail(BSG_E_INVALID, "null argument");
    Device &d = *ctx->devs[0];
    if (int32_t rc = use_device(d)) return rc;
    const hipError_t e = hipHostRegister(ptr, n_bytes, hipHostRegisterPortable);
    if (e != hipSuccess) return fail(BSG_E_HIP, "hipHostRegister: %s", hipGetErrorString(e));
    return BSG_OK;
}

int32_t bsg_host_unregister(bsg_ctx *ctx, void *ptr)
{
    BSG_ENTER(ctx);
    if (!ptr) return BSG_OK;
    HIP_TRY(hipHostUnregister(ptr));
    return BSG_OK;
}

int32_t bsg_last_match_ms(bsg_ctx *ctx, float *match_ms)
{
    BSG_ENTER(ctx);
    if (!ctx || !match_ms) return fail(BSG_E_INVALID, "null argument");
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    *match_ms = ctx->last_match_ms;
    return BSG_OK;
}

}  // extern "C"
