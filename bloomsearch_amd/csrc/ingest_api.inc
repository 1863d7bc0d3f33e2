// ingest_api.inc — C-ABI entry points of the device ingest path (included by bloomgpu.hip, which owns the
// context types).  Kernels: ingest.hip.h.
//
// One ingest = the partition buffers ("sets") of one flush or merge (flush.go:191-254: partitions are independent) and
// their file-level unions ("parents", flush.go:221,253).  On a context over several devices a call large enough is cut
// into PARTS — contiguous runs of sets, about equal in row bytes, one per device, each walked / deduplicated / built on a
// thread of its own.  A parent whose children sit in several parts is first unioned per part (a partial file-level set
// per device); the partials then travel, densely packed, device to device onto the first part's device and are unioned
// there (SURVEY 8e: "gather distinct base-hash tuples into one GPU").  Counts, bitsets and section bytes are the same
// whatever the number of parts (tests/test_shard_write_gpu.py).

namespace {

using bsg::IngestTable;
using bsh::kSlotBytes;                // four base hashes + the keyed fingerprint; every size and layout rule: host/ingest_plan.hpp

struct IngestPart {
    Device *dev;
    Scratch mem;                              // every device block the part keeps: slot storage (initial chunk + grown tables + parents) and the d_ arrays
    explicit IngestPart(Device &d) : dev(&d), mem(d) {}
    uint32_t set0 = 0, row0 = 0;              // first set / first row of this part in the caller's numbering
    uint32_t n_rows = 0, n_sets = 0, n_parents = 0;
    std::vector<uint32_t> parent_of_set;
    std::vector<IngestTable> tables;          // host mirror of d_tables [(n_sets + n_parents) * 3]
    uint64_t slot_bytes = 0;                  // HBM held by slot storage
    IngestTable *d_tables = nullptr;
    uint32_t *d_counts = nullptr, *d_status = nullptr;
    uint32_t *d_set_first = nullptr, *d_nfb = nullptr;
    uint32_t table_cap = 0;                   // (streaming) descriptors / counters d_tables, d_counts, d_status have room for
    std::vector<uint32_t> fallback;           // part-local row indices
    std::vector<uint32_t> counts, status;     // last read back
    bool finished = false;
    bsg_ingest_stats stats{};
    const bsg::MinMaxFields *mm = nullptr;    // the ingest was opened with MinMax fields (Ingest::mm_fields): k_minmax_rows runs once per upload chunk
    bsg::MinMaxRec *d_mm = nullptr;           // [mm_cap * mm->n]: per (set, field), folded over every walk so far
    uint32_t mm_cap = 0;                      // sets d_mm has room for
    float ms_minmax = 0.f;                    // k_minmax_rows dispatch time of the last call
    uint32_t n_tables() const { return (n_sets + n_parents) * 3; }
};

// A keyed ingest (bsg_ingest_open_keyed; partition.hip.h): every set has a text, set s = keys[s].  The dictionary the kernels read
// is rebuilt here from the texts and sent whole whenever it changes (a few keys per batch at most).
struct PartitionKeys {
    bsg::PkeyName name{};
    uint32_t parent = 0xFFFFFFFFu;            // of every set the ingest creates
    std::vector<std::string> keys;
    std::unordered_map<std::string, uint32_t> set_of_key;
    std::vector<bsg::PkeyDictEntry> dict;     // host mirror of d_dict
    std::vector<uint8_t> pool;                // ... and of d_pool: the texts back to back
    bsg::PkeyDictEntry *d_dict = nullptr;
    uint8_t *d_pool = nullptr;
    bsg::PkeyPending *d_pending = nullptr;
    uint32_t dict_cap = 0;
    uint64_t pool_cap = 0;
    uint32_t built_mask = 0;                  // the hash mask the tags on the device were made with
    bool dirty = true;                        // the device holds no dictionary, or not the one of `keys`
};

struct Ingest {
    std::unique_ptr<PartitionKeys> keyed;     // made by bsg_ingest_open_keyed
    uint32_t n_rows = 0, n_sets = 0, n_parents = 0;
    std::vector<uint32_t> parent_of_set;
    std::vector<std::shared_ptr<IngestPart>> parts;
    std::vector<uint32_t> set_cut;            // part p owns sets [set_cut[p], set_cut[p + 1])
    std::shared_ptr<IngestPart> merged;       // the parents, unioned across parts on the first part's device (several parts only)
    std::vector<uint32_t> fallback;           // caller's row indices, ascending
    std::vector<uint32_t> counts, status;     // caller's numbering: sets, then parents
    bsg_tokenizer tok{};                      // the spec the rows were tokenized with (bsg_ingest_rows_tok; default otherwise)
    bool streaming = false;                   // made by bsg_ingest_open: one part, rows arrive through bsg_ingest_append_rows
    uint32_t flags = 0;                       // (streaming) BSG_INGEST_* of bsg_ingest_open, applied to every append
    bsg::TokSpec spec{};                      // (streaming) the kernels' form of tok; tok_default: the default tokenizer's kernels serve
    bool tok_default = true;
    bool has_mm = false;                      // made by bsg_ingest_rows_minmax / bsg_ingest_open_minmax
    bsg::MinMaxFields mm_fields{};
    bool finished = false;
    float ms_merge = 0.f, ms_build = 0.f, ms_encode = 0.f;
    uint32_t n_tables() const { return (n_sets + n_parents) * 3; }
    uint32_t part_of_set(uint32_t s) const { return (uint32_t)(std::upper_bound(set_cut.begin(), set_cut.end(), s) - set_cut.begin()) - 1; }
};

void free_part(IngestPart &g)                 // caller holds the device lock
{
    (void)hipSetDevice(g.dev->id);
    g.mem.clear();
    g.d_tables = nullptr; g.d_counts = g.d_status = nullptr;
    g.d_set_first = g.d_nfb = nullptr;
    g.d_mm = nullptr; g.mm_cap = 0;
}

void free_ingest(Ingest &g)
{
    for (auto &p : g.parts) if (p) { std::lock_guard<std::mutex> lk(p->dev->mu); free_part(*p); }
    if (g.merged) { std::lock_guard<std::mutex> lk(g.merged->dev->mu); free_part(*g.merged); }
    g.parts.clear();
    g.merged.reset();
}

// unicode.ToLower for code points < 0x20000 as a direct table (0 = unchanged, 0xFFFFFFFF = unknown to these tables: the row
// goes to the host), from the table the host walker folds with
const std::vector<uint32_t> &lower_table()
{
    static const std::vector<uint32_t> tab = [] {
        std::vector<uint32_t> t(0x20000, 0u);
        for (const bsh::LowerPair &p : bsh::kLowerTable)
            if (p.from != p.to && p.from < 0x20000u) t[p.from] = p.to;
        for (const bsh::RuneRange &r : bsh::kUnknownRanges)
            for (uint32_t cp = r.from; cp <= r.to && cp < 0x20000u; ++cp) t[cp] = 0xFFFFFFFFu;
        return t;
    }();
    return tab;
}

int32_t ensure_lower_table(Device &d)
{
    if (d.d_lower) return BSG_OK;
    uint32_t *t = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&t), lower_table().size() * 4));
    if (hipError_t e = hipMemcpyAsync(t, lower_table().data(), lower_table().size() * 4, hipMemcpyHostToDevice, d.stream); e != hipSuccess) {
        (void)hipFree(t);                                  // (a table that never arrived must not be taken for one that did)
        return fail(BSG_E_HIP, "lower-case table: %s", hipGetErrorString(e));
    }
    d.d_lower = t;
    return BSG_OK;
}

// BasicWhitespaceLowerTokenizer as a spec: tab, LF, VT, FF, CR, space; UNICODE_SPACE | LOWER
bsg_tokenizer default_tokenizer()
{
    bsg_tokenizer t{};
    t.sep_ascii[0] = (1ull << 9) | (1ull << 10) | (1ull << 11) | (1ull << 12) | (1ull << 13) | (1ull << 32);
    t.flags = BSG_TOK_UNICODE_SPACE | BSG_TOK_LOWER;
    return t;
}

// Checks a caller's spec and derives the kernels' bitmaps (ingest.hip.h TokSpec).  *is_default: the spec is the default
// tokenizer's (NULL included), which the existing kernels serve.
int32_t tok_spec(const bsg_tokenizer *in, bsg_tokenizer &rec, bsg::TokSpec &out, bool &is_default)
{
    rec = in ? *in : default_tokenizer();
    if (rec.sep_ascii[0] & 1u) return fail(BSG_E_INVALID, "tokenizer: NUL cannot be a separator");
    if (rec.reserved) return fail(BSG_E_INVALID, "tokenizer: reserved must be 0");
    if (rec.flags & ~(BSG_TOK_UNICODE_SPACE | BSG_TOK_LOWER | BSG_TOK_NGRAM_MASK)) return fail(BSG_E_INVALID, "tokenizer: unknown flags 0x%x", rec.flags);
    const uint32_t ngram = (rec.flags & BSG_TOK_NGRAM_MASK) >> BSG_TOK_NGRAM_SHIFT;
    if (ngram == 1u || ngram > 4u) return fail(BSG_E_INVALID, "tokenizer: n-gram width %u (0, 2, 3 or 4)", ngram);
    const bsg_tokenizer d = default_tokenizer();
    is_default = rec.sep_ascii[0] == d.sep_ascii[0] && rec.sep_ascii[1] == d.sep_ascii[1] && rec.flags == d.flags;   // (a width is not the default)
    const bool lower = rec.flags & BSG_TOK_LOWER;
    auto bit = [&](uint32_t c) { return (rec.sep_ascii[c >> 6] >> (c & 63u)) & 1u; };
    out = bsg::TokSpec{};
    out.flags = rec.flags & (BSG_TOK_UNICODE_SPACE | BSG_TOK_LOWER);
    out.ngram = ngram;                        // non-zero: the _gram walkers (TokGramP)
    for (uint32_t c = 1; c < 128; ++c) {
        const uint32_t folded = (lower && c - 'A' < 26u) ? c + 32 : c;
        const uint64_t b = bit(folded);
        out.low[c >> 6] |= (uint64_t)bit(c) << (c & 63u);
        out.raw[c >> 6] |= b << (c & 63u);
        if (c >= 0x20u && c != 0x7Fu && c != '"' && c != '\\') out.run[c >> 6] |= b << (c & 63u);
    }
    return BSG_OK;
}

IngestTable as_table(const bsh::TablePlace &p) { return IngestTable{p.slots, p.fps, p.mask, p.shift}; }

// Zeroed slot storage for the tables of `lay`, one block of g.mem (of min_slots at least); their descriptors go to tables[first ...].
// counted: the block is table storage (the part's table bytes).  Caller holds the device lock and words the failure.
hipError_t alloc_tables(IngestPart &g, const bsh::TableLayout &lay, std::vector<IngestTable> &tables, size_t first, uint64_t min_slots = 0,
                        bool counted = true)
{
    void *chunk = nullptr;
    const uint64_t bytes = std::max(lay.total_slots, min_slots) * kSlotBytes;
    if (hipError_t e = g.mem.alloc(&chunk, bytes); e != hipSuccess) return e;
    if (counted) g.slot_bytes += bytes;
    for (size_t i = 0; i < lay.cap.size(); ++i) tables[first + i] = as_table(lay.place(chunk, i));
    return hipMemsetAsync(chunk, 0, lay.bytes(), g.dev->stream);
}

// A parent's tables get their storage in the finish step, sized from the children's exact counts; until then every one of them
// (tables[first ...]) is the same placeholder nothing inserts into: not table storage.
hipError_t alloc_placeholder(IngestPart &g, std::vector<IngestTable> &tables, size_t first)
{
    const hipError_t e = alloc_tables(g, bsh::layout_tables({bsh::kMinTableSlots}), tables, first, 0, false);
    std::fill(tables.begin() + first + 1, tables.end(), tables[first]);
    return e;
}

int32_t push_tables(IngestPart &g)
{
    HIP_TRY(hipMemcpyAsync(g.d_tables, g.tables.data(), g.tables.size() * sizeof(IngestTable), hipMemcpyHostToDevice, g.dev->stream));
    return BSG_OK;
}

int32_t read_state(IngestPart &g)
{
    g.counts.resize(g.n_tables());
    g.status.resize(g.n_tables());
    if (g.n_tables() == 0) return BSG_OK;
    HIP_TRY(hipMemcpyAsync(g.counts.data(), g.d_counts, g.n_tables() * 4, hipMemcpyDeviceToHost, g.dev->stream));
    HIP_TRY(hipMemcpyAsync(g.status.data(), g.d_status, g.n_tables() * 4, hipMemcpyDeviceToHost, g.dev->stream));
    HIP_TRY(hipStreamSynchronize(g.dev->stream));
    return BSG_OK;
}

// Grows every table whose status is "overflow" (x4, rehashing what it holds) and clears the flag.
// Returns the number of tables grown in *grown; tables flagged exotic are left alone.
int32_t grow_overflowed(IngestPart &g, uint32_t first, uint32_t last, uint32_t *grown)
{
    *grown = 0;
    std::vector<bsg::UnionItem> items;
    std::vector<IngestTable> fresh = g.tables;
    for (uint32_t t = first; t < last; ++t) {
        if (g.status[t] != bsg::kTableOverflow) continue;
        const uint64_t cap = bsh::grown_slots((uint64_t)g.tables[t].mask + 1);
        if (!cap) return fail(BSG_E_NOMEM, "distinct-entry table %u would exceed 2^31 slots", t);
        HIP_TRY(alloc_tables(g, bsh::layout_tables({cap}), fresh, t));
        items.push_back({t, t});
    }
    if (items.empty()) return BSG_OK;
    // old tables stay where d_tables points; the fresh ones go to a temporary descriptor array
    Scratch scratch(*g.dev);
    IngestTable *d_fresh = nullptr;
    bsg::UnionItem *d_items = nullptr;
    HIP_TRY(scratch.alloc(&d_fresh, fresh.size() * sizeof(IngestTable)));
    HIP_TRY(scratch.alloc(&d_items, items.size() * sizeof(bsg::UnionItem)));
    HIP_TRY(hipMemcpyAsync(d_fresh, fresh.data(), fresh.size() * sizeof(IngestTable), hipMemcpyHostToDevice, g.dev->stream));
    HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::UnionItem), hipMemcpyHostToDevice, g.dev->stream));
    for (auto &it : items) {   // counts restart from zero: the rehash re-counts what it moves
        HIP_TRY(hipMemsetAsync(g.d_counts + it.dst, 0, 4, g.dev->stream));
        HIP_TRY(hipMemsetAsync(g.d_status + it.dst, 0, 4, g.dev->stream));
    }
    hipLaunchKernelGGL(bsg::k_ingest_union, dim3(64, (uint32_t)items.size()), dim3(256), 0, g.dev->stream,
                       g.d_tables, d_fresh, d_items, g.d_counts, g.d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.dev->stream));
    scratch.done();
    g.tables = fresh;
    if (int32_t rc2 = push_tables(g)) return rc2;
    *grown = (uint32_t)items.size();
    return BSG_OK;
}

// Runs `launch` until no table it touches reports overflow (inserts are idempotent, so a re-run after
// growing only repeats work).  ms accumulates the kernel's own dispatch time.
template <class Launch>
int32_t run_until_fits(IngestPart &g, uint32_t first, uint32_t last, float *ms, Launch &&launch)
{
    EventList ev;                          // start / stop of the dispatch
    HIP_TRY(ev.add(2));
    for (int attempt = 0; attempt < 12; ++attempt) {
        if (int32_t rc = launch(ev.v[0], ev.v[1])) return rc;
        HIP_TRY(hipGetLastError());
        if (int32_t rc = read_state(g)) return rc;
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev.v[0], ev.v[1]));
        *ms += t;
        uint32_t grown = 0;
        if (int32_t rc = grow_overflowed(g, first, last, &grown)) return rc;
        if (!grown) return BSG_OK;
        g.stats.table_grows += grown;
    }
    return fail(BSG_E_NOMEM, "distinct-entry tables still overflow after 12 growth rounds");
}

void free_all_ingests(bsg_ctx *ctx)
{
    for (auto &kv : ctx->ingests) free_ingest(*kv.second);
    ctx->ingests.clear();
}

int32_t get_ingest(bsg_ctx *ctx, uint64_t id, std::shared_ptr<Ingest> &out)
{
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    auto it = ctx->ingests.find(id);
    if (it == ctx->ingests.end()) return fail(BSG_E_NOTFOUND, "unknown ingest id %llu", (unsigned long long)id);
    out = it->second;
    return BSG_OK;
}

// The chunk loop of a row walk (bsg_ingest_rows' parts and bsg_ingest_append_rows): chunk c + 1 travels on the copy stream while
// the compute stream walks chunk c, and a chunk is walked again after a table it overflowed has grown.  a: the launch arguments
// but for the tables and the row range; tables [0, n_set_tables) are inserted into.  stage(c), right before chunk c's bytes are
// enqueued, sends along what must have landed with them (on up.cs: the chunk's landed event covers it); launch(b, grid, e0, e1)
// enqueues the walker over b on d.stream; once(c, rf, re) runs ONCE per chunk, right after the chunk's bytes are known to land before
// it and before the chunk's first walk, never again when the walk is re-run (the MinMax scanner: its fold is not rewound).
// Caller holds the device lock; G.d_nfb has been zeroed on d.stream.
template <class Stage, class Launch, class Once>
int32_t walk_chunks(Device &d, IngestPart &G, RowUpload &up, const bsg::IngestArgs &a, uint32_t n_set_tables, const LabTrace &trace,
                    Stage &&stage, Launch &&launch, Once &&once)
{
    const uint32_t n_chunks = up.n_chunks();
    HIP_TRY(up.start(true));
    HIP_TRY(stage(0));
    HIP_TRY(up.copy(0));
    trace.lap("first chunk enqueued");
    for (uint32_t c = 0; c < n_chunks; ++c) {
        bool first_attempt = true;
        const uint32_t rf = up.cuts[c], re = up.cuts[c + 1];
        uint32_t nfb_before = 0;
        if (c) HIP_TRY(hipMemcpy(&nfb_before, G.d_nfb, 4, hipMemcpyDeviceToHost));   // K(c-1) has been synchronised
        int32_t rc = run_until_fits(G, 0, n_set_tables, &G.stats.ms_walk, [&](hipEvent_t e0, hipEvent_t e1) -> int32_t {
            if (!first_attempt) HIP_TRY(hipMemcpyAsync(G.d_nfb, &nfb_before, 4, hipMemcpyHostToDevice, d.stream));   // a re-run lists its rows again
            else {
                HIP_TRY(up.wait_landed(c));
                if (int32_t rc2 = once(c, rf, re)) return rc2;
            }
            bsg::IngestArgs b = a;
            b.tables = G.d_tables;
            b.row_first = rf; b.row_end = re;
            const bsh::WaveRuns runs = bsh::wave_runs(re - rf, d.n_cus, BSG_INGEST_WPE, bsg::kIngestThreads);
            b.rows_per_wave = runs.rows_per_wave;
            launch(b, runs.grid, e0, e1);
            if (first_attempt) {
                first_attempt = false;
                if (c + 1 < n_chunks) {                          // K(c) is running: now the next chunk's bytes
                    HIP_TRY(stage(c + 1));
                    HIP_TRY(up.copy(c + 1));
                }
            }
            return BSG_OK;
        });
        if (rc) return rc;
    }
    return BSG_OK;
}

// ---- MinMax indexes (minmax.hip.h): the fields of bsg_ingest_rows_minmax / bsg_ingest_open_minmax ----

// 1 to 8 distinct names of 1 to 64 bytes, packed like bsg_hash_entries' input.  Answered before anything is launched.
int32_t minmax_fields(const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields, bsg::MinMaxFields &out)
{
    if (n_fields == 0 || n_fields > BSG_MINMAX_MAX_FIELDS)
        return fail(BSG_E_INVALID, "minmax: n_fields = %u (1 to %u)", n_fields, BSG_MINMAX_MAX_FIELDS);
    if (!field_bytes || !field_off) return fail(BSG_E_INVALID, "minmax: field_bytes / field_off is null");
    out = bsg::MinMaxFields{};
    out.n = n_fields;
    for (uint32_t f = 0; f < n_fields; ++f) {
        if (field_off[f + 1] < field_off[f]) return fail(BSG_E_INVALID, "minmax: field_off not monotone at field %u", f);
        const uint32_t len = field_off[f + 1] - field_off[f];
        if (len == 0) return fail(BSG_E_INVALID, "minmax: field %u has an empty name", f);
        if (len > BSG_MINMAX_MAX_NAME) return fail(BSG_E_INVALID, "minmax: the name of field %u has %u bytes (at most %u)", f, len, BSG_MINMAX_MAX_NAME);
        memcpy(out.name + (size_t)f * bsg::kMinMaxMaxName, field_bytes + field_off[f], len);
        out.len[f] = (uint8_t)len;
        for (uint32_t g = 0; g < f; ++g)
            if (out.len[g] == len && !memcmp(out.name + (size_t)g * bsg::kMinMaxMaxName, out.name + (size_t)f * bsg::kMinMaxMaxName, len))
                return fail(BSG_E_INVALID, "minmax: fields %u and %u have the same name", g, f);
    }
    return BSG_OK;
}

// Room for n_sets sets in G.d_mm; what the sets before have folded travels along.  Everything behind them starts absent.
int32_t minmax_reserve(IngestPart &G, uint32_t n_sets, bool roomy)
{
    if (!G.mm || (G.d_mm && n_sets <= G.mm_cap)) return BSG_OK;
    const uint32_t nf = G.mm->n;
    const uint64_t room = bsh::minmax_room(n_sets, roomy, nf);
    if (!room) return fail(BSG_E_INVALID, "minmax: too many sets");
    bsg::MinMaxRec *fresh = nullptr;
    HIP_TRY(G.mem.alloc(&fresh, (size_t)room * nf * sizeof(bsg::MinMaxRec)));
    const uint32_t n_rec = (uint32_t)(room * nf);
    hipLaunchKernelGGL(bsg::k_minmax_init, dim3((n_rec + 255u) / 256u), dim3(256), 0, G.dev->stream, fresh, 0u, n_rec);
    HIP_TRY(hipGetLastError());
    if (G.d_mm && G.mm_cap)
        HIP_TRY(hipMemcpyAsync(fresh, G.d_mm, (size_t)G.mm_cap * nf * sizeof(bsg::MinMaxRec), hipMemcpyDeviceToDevice, G.dev->stream));
    G.d_mm = fresh;                           // (the block before stays with G.mem until the ingest is freed)
    G.mm_cap = (uint32_t)room;
    return BSG_OK;
}

// The scanner's side of one row walk: its own hand-back list (the walker's is rewound when a chunk is walked again; this one never
// is), one pair of events per chunk, and the launch walk_chunks runs once per chunk.
struct MinMaxWalk {
    IngestPart &G;
    bsg::MinMaxArgs a{};
    const bsg::RowsBySet *by_set = nullptr;   // NULL: RowsGrouped
    EventList ev;
    uint32_t *d_nfb = nullptr;
    explicit MinMaxWalk(IngestPart &g) : G(g) {}
    bool on() const { return G.mm != nullptr; }
    int32_t prepare(Scratch &scratch, const bsg::IngestArgs &w, uint32_t n_rows, const bsg::RowsBySet *rows_by_set)
    {
        if (!on()) return BSG_OK;
        by_set = rows_by_set;
        a.rows = w.rows; a.row_off = w.row_off; a.set_first_row = w.set_first_row;
        a.result = G.d_mm; a.n_sets = w.n_sets;
        HIP_TRY(scratch.alloc(&a.fallback_rows, std::max<size_t>(n_rows, 1) * 4));
        HIP_TRY(scratch.alloc(&d_nfb, 64));
        a.n_fallback = d_nfb;
        HIP_TRY(hipMemsetAsync(d_nfb, 0, 64, G.dev->stream));
        G.ms_minmax = 0.f;
        return BSG_OK;
    }
    int32_t launch(uint32_t rf, uint32_t re)
    {
        if (!on() || re <= rf) return BSG_OK;
        Device &d = *G.dev;
        HIP_TRY(ev.add(2));
        bsg::MinMaxArgs b = a;
        b.row_first = rf; b.row_end = re;
        const bsh::WaveRuns runs = bsh::wave_runs(re - rf, d.n_cus, 8, bsg::kMinMaxThreads);   // a contiguous run of rows per wave, as the walkers
        b.rows_per_wave = runs.rows_per_wave;
        const uint32_t grid = runs.grid, lds = bsg::minmax_lds_bytes(G.mm->n);
        hipEvent_t e0 = ev.v[ev.v.size() - 2], e1 = ev.v.back();
        if (by_set) hipExtLaunchKernelGGL(bsg::k_minmax_rows_sets, dim3(grid), dim3(bsg::kMinMaxThreads), lds, d.stream, e0, e1, 0, b, *G.mm, *by_set);
        else hipExtLaunchKernelGGL(bsg::k_minmax_rows, dim3(grid), dim3(bsg::kMinMaxThreads), lds, d.stream, e0, e1, 0, b, *G.mm);
        HIP_TRY(hipGetLastError());
        return BSG_OK;
    }
    // after the walk (d.stream synchronised): the rows the scanner did not decide join fb; ascending, each once
    int32_t merge_fallback(std::vector<uint32_t> &fb)
    {
        if (!on()) return BSG_OK;
        uint32_t n = 0;
        HIP_TRY(hipMemcpy(&n, d_nfb, 4, hipMemcpyDeviceToHost));
        const size_t before = fb.size();
        fb.resize(before + n);
        if (n) HIP_TRY(hipMemcpy(fb.data() + before, a.fallback_rows, (size_t)n * 4, hipMemcpyDeviceToHost));
        std::sort(fb.begin(), fb.end());
        fb.erase(std::unique(fb.begin(), fb.end()), fb.end());
        for (size_t i = 0; i + 1 < ev.v.size(); i += 2) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, ev.v[i], ev.v[i + 1]));
            G.ms_minmax += t;
        }
        return BSG_OK;
    }
};

// The six walkers by bsh::walker_slot: rows grouped by set (bsg_ingest_rows) or in a staged order (bsg_ingest_append_rows), each under
// the default tokenizer, a spec, or a spec with an n-gram width.
struct WalkerCall { uint32_t grid; hipStream_t s; hipEvent_t e0, e1; const bsg::IngestArgs &b; const bsg::RowsBySet *by_set; const bsg::TokSpec *tok; };
template <class... A> void walker(const WalkerCall &c, void (*kernel)(A...), A... a)
{
    hipExtLaunchKernelGGL(kernel, dim3(c.grid), dim3(bsg::kIngestThreads), bsg::kIngestLdsBytes, c.s, c.e0, c.e1, 0, a...);
}
void (*const kIngestWalkers[bsh::kWalkerSlots])(const WalkerCall &) = {
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows, c.b); },
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows_tok, c.b, *c.tok); },
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows_gram, c.b, *c.tok); },
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows_sets, c.b, *c.by_set); },
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows_sets_tok, c.b, *c.by_set, *c.tok); },
    [](const WalkerCall &c) { walker(c, bsg::k_ingest_rows_sets_gram, c.b, *c.by_set, *c.tok); },
};
void launch_walker(const WalkerCall &c) { kIngestWalkers[bsh::walker_slot(c.by_set != nullptr, c.tok != nullptr, c.tok && c.tok->ngram)](c); }

// One row walk — a part of bsg_ingest_rows, a batch of bsg_ingest_append_rows: the rows' device buffers, the launch arguments, the
// MinMax scanner beside the walkers, the chunk loop, the hand-back list.  The caller brings what the two differ in: the rows form
// (by_set NULL: grouped by G.d_set_first; else the order that stage(rf, re, copy stream) sends along with each chunk's bytes) and
// the upload `up` (chunked; or resident, after the partition pass a keyed batch runs between buffers() and walk()).
// Caller holds the device lock.
struct RowWalk {
    bsg_ctx *ctx; IngestPart &G; Device &d;
    const LabTrace &trace;                 // the caller's, started before it waited for the device
    const uint64_t *row_off; const uint32_t n_rows;
    Scratch scratch;                       // this call's only: the row bytes, their offsets, the hand-back list, what the caller adds
    uint8_t *d_rows = nullptr; uint64_t *d_row_off = nullptr; uint32_t *d_fb = nullptr;
    std::optional<RowUpload> up;
    RowWalk(bsg_ctx *c, IngestPart &g, const LabTrace &t, const uint64_t *off, uint32_t n)
        : ctx(c), G(g), d(*g.dev), trace(t), row_off(off), n_rows(n), scratch(*g.dev) {}
    // the row bytes end in a zeroed 64-byte tail; G.d_nfb starts at zero
    int32_t buffers()
    {
        const uint64_t n_bytes = row_off[n_rows];
        HIP_TRY(scratch.alloc(&d_rows, n_bytes + 64));
        HIP_TRY(scratch.alloc(&d_row_off, ((size_t)n_rows + 1) * 8));
        HIP_TRY(scratch.alloc(&d_fb, std::max<size_t>(n_rows, 1) * 4));
        trace.lap("device buffers allocated");
        HIP_TRY(hipMemsetAsync(d_rows + n_bytes, 0, 64, d.stream));
        HIP_TRY(hipMemcpyAsync(d_row_off, row_off, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemsetAsync(G.d_nfb, 0, 128, d.stream));
        return BSG_OK;
    }
    // Walks `up`'s rows into the sets' tables and returns with both streams synchronised; the rows handed back (the walkers' and the
    // scanner's) join fb, which leaves ascending (with fields, merge_fallback also drops a row both listed).
    template <class Stage>
    int32_t walk(uint32_t flags, const bsg::TokSpec *tok, const bsg::RowsBySet *by_set, Stage &&stage, std::vector<uint32_t> &fb)
    {
        bsg::IngestArgs a{};
        a.rows = d_rows; a.row_off = d_row_off; a.set_first_row = by_set ? nullptr : G.d_set_first;
        a.counts = G.d_counts; a.status = G.d_status; a.fallback_rows = d_fb; a.n_fallback = G.d_nfb;
        a.n_rows = n_rows; a.n_sets = G.n_sets; a.validate = (flags & BSG_INGEST_TRUSTED_JSON) ? 0u : 1u;
        a.key = ctx->fp_key;
        if (int32_t rc = ensure_lower_table(d)) return rc;
        a.lower = d.d_lower;
        MinMaxWalk mmw(G);
        if (int32_t rc = mmw.prepare(scratch, a, n_rows, by_set)) return rc;
        if (up->cuts.back())
        if (int32_t rc = walk_chunks(d, G, *up, a, G.n_sets * 3, trace,
                [&](uint32_t c) -> hipError_t { return stage(up->cuts[c], up->cuts[c + 1], up->cs); },
                [&](const bsg::IngestArgs &b, uint32_t grid, hipEvent_t e0, hipEvent_t e1) { launch_walker({grid, d.stream, e0, e1, b, by_set, tok}); },
                [&](uint32_t, uint32_t rf, uint32_t re) { return mmw.launch(rf, re); })) return rc;
        HIP_TRY(hipStreamSynchronize(d.stream));
        if (d.copy_stream) HIP_TRY(hipStreamSynchronize(d.copy_stream));
        trace.lap("all chunks walked");
        uint32_t nfb = 0;
        HIP_TRY(hipMemcpy(&nfb, G.d_nfb, 4, hipMemcpyDeviceToHost));
#ifdef BSG_INGEST_PROF
        {
            uint64_t prof[9] = {0};
            HIP_TRY(hipMemcpy(prof, G.d_nfb, 72, hipMemcpyDeviceToHost));
            const double waves = (n_rows + 63) / 64;
            fprintf(stderr, "[ingest prof] per 64-row tile: validate %.0f cyc, parse %.0f, hash %.0f, insert %.0f; rounds %.1f, insert rounds %.1f; "
                            "walker trips %.0f (slowest lane per round), %.0f (mean lane)\n",
                    prof[1] / waves, prof[2] / waves, prof[3] / waves, prof[4] / waves, prof[5] / waves, prof[6] / waves, prof[7] / waves,
                    prof[8] / waves / 64.0);
        }
#endif
        const size_t before = fb.size();
        fb.resize(before + nfb);
        if (nfb) HIP_TRY(hipMemcpy(fb.data() + before, d_fb, (size_t)nfb * 4, hipMemcpyDeviceToHost));
        std::sort(fb.begin(), fb.end());
        return mmw.merge_fallback(fb);
    }
};

// One part: rows [0, n_rows) of `rows` (row_off relative to `rows`), n_sets sets, on device d.
int32_t ingest_rows_part(bsg_ctx *ctx, Device &d, IngestPart &G, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                         const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                         const uint32_t *slots_hint, uint32_t flags, const bsg::TokSpec *tok)
{
    const LabTrace trace{"bsg_ingest_rows", d.id};
    G.n_rows = n_rows; G.n_sets = n_sets; G.n_parents = n_parents;
    G.parent_of_set.assign(n_sets, 0xFFFFFFFFu);
    if (parent_of_set) G.parent_of_set.assign(parent_of_set, parent_of_set + n_sets);
    d.calls.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    // What only this call needs on the device (the row bytes) is w.scratch; what the part keeps is G.mem, declared idle at the
    // successful end only: a failed call's parts are emptied by ingest_rows_call (free_ingest), drained first like any Scratch.
    RowWalk w(ctx, G, trace, row_off, n_rows);
    const uint32_t nt = G.n_tables();
    G.tables.assign(nt, IngestTable{nullptr, nullptr, 0, 0});
    std::vector<uint64_t> want;
    for (uint32_t s = 0; s < n_sets; ++s)
        for (uint32_t c = 0; c < 3; ++c)
            want.push_back(bsh::oneshot_slots(c, set_first_row[s + 1] - set_first_row[s], slots_hint ? slots_hint[s * 3 + c] : 0));
    HIP_TRY(alloc_tables(G, bsh::layout_tables(want), G.tables, 0, 1));
    if (n_parents) HIP_TRY(alloc_placeholder(G, G.tables, (size_t)n_sets * 3));
    HIP_TRY(G.mem.alloc(&G.d_tables, std::max<size_t>(nt, 1) * sizeof(IngestTable)));
    HIP_TRY(G.mem.alloc(&G.d_counts, std::max<size_t>(nt, 1) * 4));
    HIP_TRY(G.mem.alloc(&G.d_status, std::max<size_t>(nt, 1) * 4));
    HIP_TRY(hipMemsetAsync(G.d_counts, 0, std::max<size_t>(nt, 1) * 4, d.stream));
    HIP_TRY(hipMemsetAsync(G.d_status, 0, std::max<size_t>(nt, 1) * 4, d.stream));
    if (nt) if (int32_t rc = push_tables(G)) return rc;
    HIP_TRY(G.mem.alloc(&G.d_set_first, ((size_t)n_sets + 1) * 4));
    HIP_TRY(G.mem.alloc(&G.d_nfb, 128));
    if (int32_t rc = w.buffers()) return rc;
    HIP_TRY(hipMemcpyAsync(G.d_set_first, set_first_row, ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, d.stream));
    G.stats.n_rows = n_rows; G.stats.row_bytes = row_off[n_rows];
    if (int32_t rc = minmax_reserve(G, n_sets, false)) return rc;
    if (n_rows) {
        // The rows travel in chunks on the copy stream while the compute stream walks the chunk before (RowUpload)
        w.up.emplace(d, rows, w.d_rows, row_off, n_rows, ctx->ingest_chunk_bytes);
        if (int32_t rc = w.walk(flags, tok, nullptr, [](uint32_t, uint32_t, hipStream_t) { return hipSuccess; }, G.fallback)) return rc;
    } else if (int32_t rc = read_state(G)) return rc;
    G.stats.n_fallback_rows = (uint32_t)G.fallback.size();
    // both streams have been synchronised: the row bytes leave the device with the walk's scratch, the part keeps the rest
    w.scratch.done();
    G.mem.done();
    return BSG_OK;
}

// The file-level union through global hash tables (round 2's path): every child entry is CAS-inserted into a parent table of
// 2 x the children's entries.  Kept as the fallback of union_partitioned (a key distribution the partitions cannot split).
int32_t union_global_tables(IngestPart &G, const std::vector<uint64_t> &sum, const std::vector<bsg::UnionItem> &items)
{
    Device &d = *G.dev;
    // parent capacity from the exact child counts: 2 x (sum of children) bounds the union, so it cannot overflow
    std::vector<uint64_t> want;
    for (uint64_t s : sum) want.push_back(bsh::parent_slots(s));
    HIP_TRY(alloc_tables(G, bsh::layout_tables(want), G.tables, (size_t)G.n_sets * 3));
    if (int32_t rc = push_tables(G)) return rc;
    if (items.empty()) return BSG_OK;
    Scratch scratch(d);
    bsg::UnionItem *d_items = nullptr;
    HIP_TRY(scratch.alloc(&d_items, items.size() * sizeof(bsg::UnionItem)));
    HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::UnionItem), hipMemcpyHostToDevice, d.stream));
    if (int32_t rc = run_until_fits(G, G.n_sets * 3, G.n_tables(), &G.stats.ms_union, [&](hipEvent_t e0, hipEvent_t e1) -> int32_t {
            hipExtLaunchKernelGGL(bsg::k_ingest_union, dim3(64, (uint32_t)items.size()), dim3(256), 0, d.stream, e0, e1, 0,
                                  G.d_tables, G.d_tables, d_items, G.d_counts, G.d_status);
            return BSG_OK;
        })) return rc;
    scratch.done();                        // run_until_fits returns synchronised
    return BSG_OK;
}

// The file-level union partition by partition in LDS (k_union_partitions): dense parents of exactly the distinct entries,
// 40 bytes of output room per CHILD entry, no memset, one global atomic per workgroup.  *fell_back: the partitions could not
// be made fine enough (a few retries with 4 x more of them) — the caller takes the global tables instead.
int32_t union_partitioned(IngestPart &G, const std::vector<uint64_t> &sum, const std::vector<bsg::UnionItem> &items, bool *fell_back, uint32_t coarsen)
{
    *fell_back = false;
    Device &d = *G.dev;
    const uint32_t P3 = G.n_parents * 3;
    // children per parent table, grouped
    std::vector<std::vector<uint32_t>> kids(P3);
    for (const bsg::UnionItem &it : items) kids[it.dst - G.n_sets * 3].push_back(it.src);
    std::vector<uint32_t> child_list;
    std::vector<bsg::PartParent> parents(P3);
    const bsh::TableLayout lay = bsh::layout_tables(sum, true);      // dense: room for every child entry, no memset
    if (lay.total_slots == 0) return push_tables(G);       // every parent is empty: the placeholders stay
    if (lay.total_slots > bsh::kMaxTableSlots) { *fell_back = true; return BSG_OK; }
    void *chunk = nullptr;
    HIP_TRY(G.mem.alloc(&chunk, lay.bytes()));
    G.slot_bytes += lay.bytes();
    for (uint32_t t = 0; t < P3; ++t) {
        bsg::PartParent &pp = parents[t];
        const bsh::TablePlace out = lay.place(chunk, t);
        pp.out_slots = out.slots;
        pp.out_fps = out.fps;
        pp.cap_out = (uint32_t)sum[t];
        pp.child_begin = (uint32_t)child_list.size();
        child_list.insert(child_list.end(), kids[t].begin(), kids[t].end());
        pp.child_end = (uint32_t)child_list.size();
        pp.table = G.n_sets * 3 + t;
        pp.log2P = bsh::first_log2P(sum[t], bsg::kPartTarget, coarsen);
    }
    uint32_t *d_kids = nullptr;
    bsg::PartParent *d_parents = nullptr;
    Scratch scratch(d);
    HIP_TRY(scratch.alloc(&d_kids, std::max<size_t>(child_list.size(), 1) * 4));
    HIP_TRY(scratch.alloc(&d_parents, parents.size() * sizeof(bsg::PartParent)));
    if (!child_list.empty()) HIP_TRY(hipMemcpyAsync(d_kids, child_list.data(), child_list.size() * 4, hipMemcpyHostToDevice, d.stream));
    EventList ev;                          // start / stop of the dispatch
    HIP_TRY(ev.add(2));
    // `todo`: the parents this attempt launches — all of them first, then only those whose partitioning was too coarse (their
    // records are the first todo.size() entries of d_parents; the kernel reaches counts / status / output through pp.table, so
    // the finished parents keep their counts and their dense lists while the others are repeated 4 x finer)
    std::vector<uint32_t> todo(P3);
    for (uint32_t t = 0; t < P3; ++t) todo[t] = t;
    std::vector<bsg::PartParent> launch;
    for (int attempt = 0; attempt < 4; ++attempt) {
        launch.clear();
        uint32_t max_log2P = 0;
        for (uint32_t t : todo) { launch.push_back(parents[t]); max_log2P = std::max(max_log2P, parents[t].log2P); }
        HIP_TRY(hipMemcpyAsync(d_parents, launch.data(), launch.size() * sizeof(bsg::PartParent), hipMemcpyHostToDevice, d.stream));
        if (todo.size() == P3) HIP_TRY(hipMemsetAsync(G.d_counts + G.n_sets * 3, 0, (size_t)P3 * 4, d.stream));
        else for (uint32_t t : todo) HIP_TRY(hipMemsetAsync(G.d_counts + G.n_sets * 3 + t, 0, 4, d.stream));
        hipExtLaunchKernelGGL(bsg::k_union_partitions, dim3(1u << max_log2P, (uint32_t)todo.size()), dim3(bsg::kPartThreads), bsg::kPartLdsBytes, d.stream, ev.v[0], ev.v[1], 0,
                              (const IngestTable *)G.d_tables, (const uint32_t *)d_kids, (const bsg::PartParent *)d_parents, G.d_counts, G.d_status);
        HIP_TRY(hipGetLastError());
        if (int32_t rc = read_state(G)) return rc;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.v[0], ev.v[1]));
        G.stats.ms_union += ms;
        bool again = false;
        std::vector<uint32_t> next;
        for (uint32_t t : todo) {
            if (G.status[G.n_sets * 3 + t] != bsg::kTableOverflow) continue;
            again = true;
            next.push_back(t);
            parents[t].log2P = bsh::finer_log2P(parents[t].log2P);
        }
        todo.swap(next);
        if (!again) {
            for (uint32_t t = 0; t < P3; ++t) {
                const uint32_t n = G.counts[G.n_sets * 3 + t];
                if (n) G.tables[G.n_sets * 3 + t] = as_table(bsh::place_table(chunk, lay.first_slot[t], lay.total_slots, n, true));      // a dense list
            }
            scratch.done();                // read_state has synchronised; push_tables touches neither list
            return push_tables(G);
        }
        // only the overflowed parents' status is cleared: exotic flags of the others (and theirs) must survive
        for (uint32_t t = 0; t < P3; ++t)
            if (G.status[G.n_sets * 3 + t] == bsg::kTableOverflow) HIP_TRY(hipMemsetAsync(G.d_status + G.n_sets * 3 + t, 0, 4, d.stream));
        G.stats.table_grows += 1;
    }
    // not splittable (an adversarial key distribution): clear what this path left behind and let the global tables do it
    HIP_TRY(hipMemsetAsync(G.d_counts + G.n_sets * 3, 0, (size_t)P3 * 4, d.stream));
    HIP_TRY(hipMemsetAsync(G.d_status + G.n_sets * 3, 0, (size_t)P3 * 4, d.stream));
    scratch.done();                        // the last attempt's read_state has synchronised; the memsets touch neither list
    *fell_back = true;
    return BSG_OK;
}

// Unions the part's sets into ITS parent tables (partial file-level sets when the ingest has several parts) and reads
// the exact counts back.
int32_t finish_part(bsg_ctx *ctx, IngestPart &G)
{
    Device &d = *G.dev;
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    if (G.finished) return BSG_OK;
    if (int32_t rc = read_state(G)) return rc;
    if (G.n_parents) {
        std::vector<uint64_t> sum((size_t)G.n_parents * 3, 0);
        std::vector<bsg::UnionItem> items;
        for (uint32_t s = 0; s < G.n_sets; ++s) {
            const uint32_t p = G.parent_of_set[s];
            if (p == 0xFFFFFFFFu) continue;
            for (uint32_t c = 0; c < 3; ++c) {
                sum[(size_t)p * 3 + c] += G.counts[s * 3 + c];
                items.push_back({s * 3 + c, (G.n_sets + p) * 3 + c});
            }
        }
        bool fell_back = ctx->union_mode == 1;             // lab knob: 1 = always the global tables
        if (!fell_back) if (int32_t rc = union_partitioned(G, sum, items, &fell_back, ctx->union_coarsen)) return rc;
        if (fell_back) if (int32_t rc = union_global_tables(G, sum, items)) return rc;
    }
    if (int32_t rc = read_state(G)) return rc;
    G.finished = true;
    return BSG_OK;
}

// The parts' partial parents -> one set of parent tables on the first part's device.  Every other part packs the occupied
// slots of its partial tables densely (k_table_compact) and they travel device to device; the first part's partials are read
// in place.  One k_ingest_union launch folds them all.
int32_t merge_parents(bsg_ctx *ctx, Ingest &I)
{
    const uint32_t np = (uint32_t)I.parts.size(), P3 = I.n_parents * 3;
    Device &H = *I.parts[0]->dev;
    struct Dense { void *buf = nullptr; uint32_t n = 0; Device *dev = nullptr; };
    std::vector<Dense> dense((size_t)np * P3);
    int32_t rc = run_parts(np - 1, [&](uint32_t i) -> int32_t {
        IngestPart &G = *I.parts[i + 1];
        Device &d = *G.dev;
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc2 = use_device(d)) return rc2;
        Scratch scratch(d);
        uint32_t *d_counter = nullptr;
        HIP_TRY(scratch.alloc(&d_counter, (size_t)P3 * 4));
        HIP_TRY(hipMemsetAsync(d_counter, 0, (size_t)P3 * 4, d.stream));
        for (uint32_t t = 0; t < P3; ++t) {
            const uint32_t n = G.counts[G.n_sets * 3 + t];
            Dense &x = dense[(size_t)(i + 1) * P3 + t];
            x.n = n; x.dev = &d;
            if (!n) continue;
            HIP_TRY(d.pool.alloc(&x.buf, (uint64_t)n * kSlotBytes));
            const IngestTable &src = G.tables[G.n_sets * 3 + t];
            const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)src.mask + 1 + 255) / 256, (uint64_t)d.n_cus * 8);
            hipLaunchKernelGGL(bsg::k_table_compact, dim3(std::max(grid, 1u)), dim3(256), 0, d.stream, src, (uint64_t *)x.buf, (uint64_t *)x.buf + (uint64_t)n * 4,
                               d_counter + t, n);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(d.stream));
        scratch.done();
        return BSG_OK;
    });
    auto M = std::make_shared<IngestPart>(H);
    M->n_sets = 0; M->n_parents = I.n_parents;
    auto merge_try = [](hipError_t e) { return e == hipSuccess ? BSG_OK : fail(e == hipErrorOutOfMemory ? BSG_E_NOMEM : BSG_E_HIP, "parent merge: %s", hipGetErrorString(e)); };
    if (!rc) {
        std::lock_guard<std::mutex> lk(H.mu);
        rc = [&]() -> int32_t {
            if (int32_t rc2 = use_device(H)) return rc2;
            Scratch copies(H);             // the other parts' dense lists on this device, and the union's two argument arrays
            // capacity: 2 x the sum of the partial counts bounds the union
            std::vector<uint64_t> want(P3, 0);
            for (uint32_t t = 0; t < P3; ++t)
                for (uint32_t q = 0; q < np; ++q) want[t] += I.parts[q]->counts[I.parts[q]->n_sets * 3 + t];
            for (uint64_t &w : want) w = bsh::parent_slots(w);
            M->tables.assign(P3, IngestTable{nullptr, nullptr, 0, 0});
            if (int32_t rc2 = merge_try(alloc_tables(*M, bsh::layout_tables(want), M->tables, 0))) return rc2;
            if (int32_t rc2 = merge_try(M->mem.alloc(&M->d_tables, (size_t)P3 * sizeof(IngestTable)))) return rc2;
            if (int32_t rc2 = merge_try(M->mem.alloc(&M->d_counts, (size_t)P3 * 4))) return rc2;
            if (int32_t rc2 = merge_try(M->mem.alloc(&M->d_status, (size_t)P3 * 4))) return rc2;
            if (int32_t rc2 = merge_try(hipMemsetAsync(M->d_counts, 0, (size_t)P3 * 4, H.stream))) return rc2;
            if (int32_t rc2 = merge_try(hipMemsetAsync(M->d_status, 0, (size_t)P3 * 4, H.stream))) return rc2;
            // sources: part 0's partial tables in place, every other part's dense copy
            std::vector<IngestTable> src((size_t)np * P3, IngestTable{nullptr, nullptr, 0, 0});
            std::vector<bsg::UnionItem> items;
            for (uint32_t t = 0; t < P3; ++t) {
                src[t] = I.parts[0]->tables[I.parts[0]->n_sets * 3 + t];
                if (I.parts[0]->counts[I.parts[0]->n_sets * 3 + t]) items.push_back({t, t});
                for (uint32_t q = 1; q < np; ++q) {
                    const Dense &x = dense[(size_t)q * P3 + t];
                    if (!x.n) continue;
                    void *cp = nullptr;
                    if (int32_t rc2 = merge_try(copies.alloc(&cp, (uint64_t)x.n * kSlotBytes))) return rc2;
                    if (int32_t rc2 = merge_try(peer_copy(ctx, dev_index(ctx, &H), cp, dev_index(ctx, x.dev), x.buf, (uint64_t)x.n * kSlotBytes, H.stream))) return rc2;
                    src[(size_t)q * P3 + t] = as_table(bsh::place_table(cp, 0, x.n, x.n, true));
                    items.push_back({q * P3 + t, t});
                }
            }
            IngestTable *d_src = nullptr;
            bsg::UnionItem *d_items = nullptr;
            if (int32_t rc2 = merge_try(copies.alloc(&d_src, src.size() * sizeof(IngestTable)))) return rc2;
            if (int32_t rc2 = merge_try(copies.alloc(&d_items, std::max<size_t>(items.size(), 1) * sizeof(bsg::UnionItem)))) return rc2;
            if (int32_t rc2 = merge_try(hipMemcpyAsync(d_src, src.data(), src.size() * sizeof(IngestTable), hipMemcpyHostToDevice, H.stream))) return rc2;
            if (!items.empty()) if (int32_t rc2 = merge_try(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::UnionItem), hipMemcpyHostToDevice, H.stream))) return rc2;
            if (int32_t rc2 = push_tables(*M)) return rc2;
            if (items.empty()) { if (int32_t rc2 = read_state(*M)) return rc2; }
            else if (int32_t rc2 = run_until_fits(*M, 0, P3, &I.ms_merge, [&](hipEvent_t e0, hipEvent_t e1) -> int32_t {
                    hipExtLaunchKernelGGL(bsg::k_ingest_union, dim3(64, (uint32_t)items.size()), dim3(256), 0, H.stream, e0, e1, 0,
                                          (const IngestTable *)d_src, (const IngestTable *)M->d_tables, (const bsg::UnionItem *)d_items, M->d_counts, M->d_status);
                    return BSG_OK;
                })) return rc2;
            // a partial that was flagged (an unrepresentable entry, a hash-equal pair) flags the merged parent too
            for (uint32_t t = 0; t < P3; ++t)
                for (uint32_t q = 0; q < np; ++q) M->status[t] = std::max(M->status[t], I.parts[q]->status[I.parts[q]->n_sets * 3 + t]);
            M->finished = true;
            copies.done();                 // run_until_fits / read_state return synchronised
            M->mem.done();
            return BSG_OK;
        }();
        if (rc) free_part(*M);             // (under H's lock)
    }
    // whatever happened above, the dense lists leave their devices here, each under its own device's lock
    for (Dense &x : dense) if (x.buf) { std::lock_guard<std::mutex> lk(x.dev->mu); (void)hipSetDevice(x.dev->id); x.dev->pool.free(x.buf); }
    if (rc) return rc;
    I.merged = M;
    return BSG_OK;
}

// What bsh::check_rows / check_set_first / check_parents found, refused in the words of the entry points
int32_t refuse(const bsh::RowCheck &c)
{
    switch (c.fault) {
    case bsh::RowFault::None: return BSG_OK;
    case bsh::RowFault::OffsetsNotMonotone: return fail(BSG_E_INVALID, "row_off not monotone at %u", c.at);
    case bsh::RowFault::BytesMissing: return fail(BSG_E_INVALID, "rows is null");
    case bsh::RowFault::SetFirstSpan: return fail(BSG_E_INVALID, "set_first_row must span [0, n_rows]");
    case bsh::RowFault::SetFirstNotMonotone: return fail(BSG_E_INVALID, "set_first_row not monotone at %u", c.at);
    case bsh::RowFault::ParentsMissing: return fail(BSG_E_INVALID, "parent_of_set is null");
    default: return fail(BSG_E_INVALID, "parent_of_set[%u] out of range", c.at);
    }
}
int32_t check_parents(const uint32_t *parent_of_set, uint32_t n_sets, uint32_t n_parents) { return refuse(bsh::check_parents(parent_of_set, n_sets, n_parents)); }
int32_t check_table_count(uint64_t n) { return bsh::too_many_tables(n) ? fail(BSG_E_INVALID, "too many sets and parents") : BSG_OK; }
// the ingest's own record of its one part's sets, after sets were added to the part
void sync_sets(Ingest &I, const IngestPart &G) { I.n_sets = G.n_sets; I.parent_of_set = G.parent_of_set; I.set_cut = {0, I.n_sets}; }

// bsg_ingest_rows (tok_in NULL) and bsg_ingest_rows_tok
int32_t ingest_rows_call(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                         const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                         const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok_in, uint64_t *out_ingest_id,
                         const bsg::MinMaxFields *mm = nullptr)
{
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    bsg_tokenizer rec{};
    bsg::TokSpec spec{};
    bool is_default = true;
    if (int32_t rc = tok_spec(tok_in, rec, spec, is_default)) return rc;
    const bsg::TokSpec *tok = is_default ? nullptr : &spec;
    if (!out_ingest_id || !row_off || !set_first_row || n_sets == 0) return fail(BSG_E_INVALID, "null argument or no sets");
    if (int32_t rc = refuse(bsh::check_set_first(set_first_row, n_sets, n_rows))) return rc;
    if (int32_t rc = refuse(bsh::check_rows(row_off, n_rows, rows != nullptr))) return rc;
    if (int32_t rc = check_parents(parent_of_set, n_sets, n_parents)) return rc;
    const uint64_t n_bytes = row_off[n_rows];

    auto I = std::make_shared<Ingest>();
    I->n_rows = n_rows; I->n_sets = n_sets; I->n_parents = n_parents;
    I->tok = rec;
    if (mm) { I->has_mm = true; I->mm_fields = *mm; }
    I->parent_of_set.assign(n_sets, 0xFFFFFFFFu);
    if (parent_of_set) I->parent_of_set.assign(parent_of_set, parent_of_set + n_sets);
    // parts: contiguous runs of sets, about equal in row bytes, one per device
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const uint32_t want = (nd > 1 && n_bytes >= ctx->shard_min_row_bytes) ? std::min(nd, n_sets) : 1;
    if (want > 1) {
        std::vector<uint64_t> cost(n_sets);
        for (uint32_t s = 0; s < n_sets; ++s) cost[s] = row_off[set_first_row[s + 1]] - row_off[set_first_row[s]] + 64;
        I->set_cut = balanced_cuts(cost, want);
    } else {
        I->set_cut = {0, n_sets};
    }
    const uint32_t np = (uint32_t)I->set_cut.size() - 1;
    const uint32_t first = np == 1 ? pick_device(ctx) : 0;
    for (uint32_t i = 0; i < np; ++i) I->parts.push_back(std::make_shared<IngestPart>(*ctx->devs[(first + i) % nd]));
    const int32_t rc = run_parts(np, [&](uint32_t i) -> int32_t {
        IngestPart &G = *I->parts[i];
        const uint32_t s0 = I->set_cut[i], s1 = I->set_cut[i + 1], r0 = set_first_row[s0], r1 = set_first_row[s1];
        G.set0 = s0; G.row0 = r0;
        G.mm = I->has_mm ? &I->mm_fields : nullptr;
        Device &d = *G.dev;
        if (np == 1)
            return ingest_rows_part(ctx, d, G, rows, row_off, n_rows, set_first_row, n_sets, parent_of_set, n_parents, slots_hint, flags, tok);
        // the part's rows and sets, renumbered from zero (offsets relative to the part's first byte)
        const uint64_t byte0 = row_off[r0];
        std::vector<uint64_t> off((size_t)(r1 - r0) + 1);
        for (uint32_t r = r0; r <= r1; ++r) off[r - r0] = row_off[r] - byte0;
        std::vector<uint32_t> sfr((size_t)(s1 - s0) + 1);
        for (uint32_t s = s0; s <= s1; ++s) sfr[s - s0] = set_first_row[s] - r0;
        return ingest_rows_part(ctx, d, G, rows ? rows + byte0 : nullptr, off.data(), r1 - r0, sfr.data(), s1 - s0, parent_of_set ? parent_of_set + s0 : nullptr,
                                n_parents, slots_hint ? slots_hint + (size_t)s0 * 3 : nullptr, flags, tok);
    });
    if (rc) { free_ingest(*I); return rc; }
    float ms_minmax = 0.f;
    for (auto &p : I->parts) {
        for (uint32_t r : p->fallback) I->fallback.push_back(r + p->row0);
        ms_minmax = std::max(ms_minmax, p->ms_minmax);
    }
    std::sort(I->fallback.begin(), I->fallback.end());
    std::lock_guard<std::shared_mutex> lk2(ctx->mu);
    if (mm) ctx->last_minmax_ms = ms_minmax;
    const uint64_t id = ctx->next_id++;
    ctx->ingests[id] = I;
    *out_ingest_id = id;
    return BSG_OK;
}


// ---- streaming ingest: bsg_ingest_open, bsg_ingest_add_sets, bsg_ingest_append_rows ----
// One part on one device.  Its tables are laid out like every part's — the sets' three tables each, then the parents' — so
// finish, build and free see nothing new.  The parents are placeholders until finish_part gives them storage and nothing is
// inserted into them before: their counters and flags are zero, so adding sets only moves their DESCRIPTORS behind the new
// sets' (the caller's numbering "sets, then parents" holds at every moment; a parent's table index is (n_sets + p) * 3 + kind
// with the n_sets of the time).

// n_more empty sets behind the existing ones.  Caller holds the device lock and has made the device current.
int32_t stream_add_sets(IngestPart &G, uint32_t n_more, const uint32_t *parent_of_new_set, const uint32_t *slots_hint)
{
    Device &d = *G.dev;
    const uint32_t old_sets = G.n_sets, new_sets = old_sets + n_more, nt = (new_sets + G.n_parents) * 3;
    std::vector<IngestTable> tables(nt, IngestTable{nullptr, nullptr, 0, 0});
    std::copy(G.tables.begin(), G.tables.begin() + (size_t)old_sets * 3, tables.begin());
    std::copy(G.tables.begin() + (size_t)old_sets * 3, G.tables.end(), tables.begin() + (size_t)new_sets * 3);   // the parents' placeholders
    if (n_more) {
        std::vector<uint64_t> want((size_t)n_more * 3);
        for (size_t i = 0; i < want.size(); ++i) want[i] = bsh::stream_slots(i % 3, slots_hint ? slots_hint[i] : 0);
        HIP_TRY(alloc_tables(G, bsh::layout_tables(want), tables, (size_t)old_sets * 3));
    }
    if (nt > G.table_cap || !G.d_tables) {
        // room for twice as many: partitions keep showing up.  The sets' counters travel; everything behind them is zero.
        const uint32_t room = bsh::descriptor_room(nt);
        IngestTable *nd_tables = nullptr;
        uint32_t *nd_counts = nullptr, *nd_status = nullptr;
        HIP_TRY(G.mem.alloc(&nd_tables, (size_t)room * sizeof(IngestTable)));
        HIP_TRY(G.mem.alloc(&nd_counts, (size_t)room * 4));
        HIP_TRY(G.mem.alloc(&nd_status, (size_t)room * 4));
        HIP_TRY(hipMemsetAsync(nd_counts, 0, (size_t)room * 4, d.stream));
        HIP_TRY(hipMemsetAsync(nd_status, 0, (size_t)room * 4, d.stream));
        if (old_sets) {
            HIP_TRY(hipMemcpyAsync(nd_counts, G.d_counts, (size_t)old_sets * 3 * 4, hipMemcpyDeviceToDevice, d.stream));
            HIP_TRY(hipMemcpyAsync(nd_status, G.d_status, (size_t)old_sets * 3 * 4, hipMemcpyDeviceToDevice, d.stream));
        }
        G.d_tables = nd_tables; G.d_counts = nd_counts; G.d_status = nd_status;   // (the blocks before stay with G.mem until the ingest is freed)
        G.table_cap = room;
    }
    G.tables.swap(tables);
    G.n_sets = new_sets;
    for (uint32_t i = 0; i < n_more; ++i) G.parent_of_set.push_back(parent_of_new_set ? parent_of_new_set[i] : 0xFFFFFFFFu);
    if (nt) if (int32_t rc = push_tables(G)) return rc;
    if (int32_t rc = minmax_reserve(G, new_sets, true)) return rc;
    HIP_TRY(hipStreamSynchronize(d.stream));
    return BSG_OK;
}

int32_t ingest_open_call(bsg_ctx *ctx, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents, const uint32_t *slots_hint,
                         uint32_t flags, const bsg_tokenizer *tok_in, uint64_t *out_ingest_id, const bsg::MinMaxFields *mm = nullptr,
                         std::unique_ptr<PartitionKeys> keyed = nullptr)
{
    auto I = std::make_shared<Ingest>();
    I->keyed = std::move(keyed);
    if (mm) { I->has_mm = true; I->mm_fields = *mm; }
    if (int32_t rc = tok_spec(tok_in, I->tok, I->spec, I->tok_default)) return rc;
    if (!out_ingest_id) return fail(BSG_E_INVALID, "null argument");
    if (flags & ~BSG_INGEST_TRUSTED_JSON) return fail(BSG_E_INVALID, "unknown flags 0x%x", flags);
    if (int32_t rc = check_table_count((uint64_t)n_sets + n_parents)) return rc;
    if (int32_t rc = check_parents(parent_of_set, n_sets, n_parents)) return rc;
    I->streaming = true;
    I->flags = flags;
    I->n_parents = n_parents;
    Device &d = *ctx->devs[pick_device(ctx)];
    auto P = std::make_shared<IngestPart>(d);
    I->parts.push_back(P);
    IngestPart &G = *P;
    G.n_parents = n_parents;
    G.mm = I->has_mm ? &I->mm_fields : nullptr;
    int32_t rc = BSG_OK;
    {
        std::lock_guard<std::mutex> lk(d.mu);
        rc = [&]() -> int32_t {
            if (int32_t rc2 = use_device(d)) return rc2;
            G.tables.assign((size_t)n_parents * 3, IngestTable{nullptr, nullptr, 0, 0});
            if (n_parents) HIP_TRY(alloc_placeholder(G, G.tables, 0));
            HIP_TRY(G.mem.alloc(&G.d_nfb, 128));
            if (int32_t rc2 = stream_add_sets(G, n_sets, parent_of_set, slots_hint)) return rc2;
            G.mem.done();                  // stream_add_sets returns synchronised
            return BSG_OK;
        }();
    }
    if (rc) { free_ingest(*I); return rc; }
    sync_sets(*I, G);
    std::lock_guard<std::shared_mutex> lk2(ctx->mu);
    const uint64_t id = ctx->next_id++;
    ctx->ingests[id] = I;
    *out_ingest_id = id;
    return BSG_OK;
}

// a streaming ingest that still takes sets and rows
int32_t get_open_stream(bsg_ctx *ctx, uint64_t id, std::shared_ptr<Ingest> &g, const char *call)
{
    if (int32_t rc = get_ingest(ctx, id, g)) return rc;
    if (!g->streaming) return fail(BSG_E_INVALID, "%s: ingest %llu was made by bsg_ingest_rows, not by bsg_ingest_open", call, (unsigned long long)id);
    if (g->finished) return fail(BSG_E_INVALID, "%s: ingest already finished", call);
    return BSG_OK;
}

// ---- keyed ingest: the dictionary and the partition pass of one batch (partition.hip.h) ----

// The dictionary over keys (set s = its index) and, behind them, `fresh` (texts this call has met and not numbered yet: their
// entries carry kPkeyProvisional | index), built on the host and sent whole.  Caller holds the device lock; d.stream is idle.
int32_t keyed_upload(IngestPart &G, PartitionKeys &K, uint32_t hash_mask, const std::vector<std::string> &fresh)
{
    Device &d = *G.dev;
    const size_t nk = K.keys.size(), n = nk + fresh.size();
    uint32_t cap = std::max<uint32_t>(64, K.dict_cap);
    while ((uint64_t)cap < (uint64_t)n * 2 + 2) cap <<= 1;      // at most half full: a lookup always meets an empty slot
    K.dict.assign(cap, bsg::PkeyDictEntry{0, 0, 0, 0});
    K.pool.clear();
    for (size_t i = 0; i < n; ++i) {
        const std::string &t = i < nk ? K.keys[i] : fresh[i - nk];
        const uint32_t tag = bsg::partition_tag_bytes(reinterpret_cast<const uint8_t *>(t.data()), (uint32_t)t.size(), hash_mask);
        uint32_t slot = tag & (cap - 1);
        while (K.dict[slot].tag) slot = (slot + 1) & (cap - 1);
        K.dict[slot] = bsg::PkeyDictEntry{tag, i < nk ? (uint32_t)i : bsg::kPkeyProvisional | (uint32_t)(i - nk), (uint32_t)K.pool.size(), (uint32_t)t.size()};
        K.pool.insert(K.pool.end(), t.begin(), t.end());
    }
    if (K.pool.size() > 0x7FFFFFFFull) return fail(BSG_E_INVALID, "keyed ingest: the partition texts exceed 2 GiB");
    if (cap > K.dict_cap || !K.d_dict) {
        HIP_TRY(G.mem.alloc(&K.d_dict, (size_t)cap * sizeof(bsg::PkeyDictEntry)));      // (the block before stays with G.mem until the ingest is freed)
        K.dict_cap = cap;
    }
    if (K.pool.size() > K.pool_cap || !K.d_pool) {
        const uint64_t room = std::max<uint64_t>(4096, K.pool.size() * 2);
        HIP_TRY(G.mem.alloc(&K.d_pool, room));
        K.pool_cap = room;
    }
    HIP_TRY(hipMemcpyAsync(K.d_dict, K.dict.data(), (size_t)cap * sizeof(bsg::PkeyDictEntry), hipMemcpyHostToDevice, d.stream));
    if (!K.pool.empty()) HIP_TRY(hipMemcpyAsync(K.d_pool, K.pool.data(), K.pool.size(), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    K.built_mask = hash_mask;
    K.dirty = false;
    return BSG_OK;
}

// the device scanner on the host's copy of one row (laid into aligned words with the look-ahead the scanner may read)
bool keyed_host_text(const PartitionKeys &K, const uint8_t *row, uint64_t len, std::string &text)
{
    std::vector<uint64_t> words((size_t)(len >> 3) + 3, 0);
    if (len) memcpy(words.data(), row, len);
    const bsg::PkeyScan sc = bsg::partition_scan_row(words.data(), 0, len, K.name.name, K.name.len);
    if (sc.undecided) return false;
    text.assign(reinterpret_cast<const char *>(words.data()) + sc.pos, sc.len);
    return true;
}

struct KeyedCall {
    uint32_t *out_set_of_row;
    uint32_t *out_n_new_sets;
    uint32_t hash_mask;
};

// The partition pass of one keyed batch: uploads the rows chunk by chunk with k_partition_rows behind each chunk, resolves the new
// texts in rounds (host: pending slots -> dictionary; device: k_partition_assign), numbers them by their lowest row, creates their
// sets and leaves: sets[r] (final numbers, kPkeyUndecided for the rows handed back), kept = the rows to walk, kept_sets their sets.
// The row bytes stay resident in d_rows.  Caller holds the device lock.
int32_t partition_batch(bsg_ctx *ctx, Ingest &I, IngestPart &G, Scratch &scratch, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                        uint8_t *d_rows, uint64_t *d_row_off, const KeyedCall &kc, std::vector<uint32_t> &sets, std::vector<uint32_t> &kept,
                        std::vector<uint32_t> &kept_sets, float *ms_partition)
{
    Device &d = *G.dev;
    PartitionKeys &K = *I.keyed;
    if (K.dirty || K.built_mask != kc.hash_mask || !K.d_dict) if (int32_t rc = keyed_upload(G, K, kc.hash_mask, {})) return rc;
    uint32_t *d_set = nullptr;
    bsg::PkeyRow *d_key = nullptr;
    HIP_TRY(scratch.alloc(&d_set, (size_t)n_rows * 4));
    HIP_TRY(scratch.alloc(&d_key, (size_t)n_rows * sizeof(bsg::PkeyRow)));
    if (!K.d_pending) HIP_TRY(G.mem.alloc(&K.d_pending, bsg::kPkeyPendingSlots * sizeof(bsg::PkeyPending)));
    const std::vector<bsg::PkeyPending> unclaimed(bsg::kPkeyPendingSlots, bsg::PkeyPending{0u, 0xFFFFFFFFu});
    HIP_TRY(hipMemcpyAsync(K.d_pending, unclaimed.data(), unclaimed.size() * sizeof(bsg::PkeyPending), hipMemcpyHostToDevice, d.stream));
    bsg::PkeyArgs a{};
    a.rows = d_rows; a.row_off = d_row_off; a.dict = K.d_dict; a.pool = K.d_pool; a.pending = K.d_pending; a.row_key = d_key; a.set_of_row = d_set;
    a.dict_mask = K.dict_cap - 1; a.hash_mask = kc.hash_mask;
    EventList ev;
    auto timed = [&](auto &&launch) -> hipError_t {
        if (hipError_t e = ev.add(2); e != hipSuccess) return e;
        launch(ev.v[ev.v.size() - 2], ev.v.back());
        return hipGetLastError();
    };
    // the scan of chunk c runs behind chunk c's bytes while chunk c + 1 travels on the copy stream
    RowUpload up(d, rows, d_rows, row_off, n_rows, ctx->ingest_chunk_bytes);
    HIP_TRY(up.start(true));
    for (uint32_t c = 0; c < up.n_chunks(); ++c) {
        HIP_TRY(up.copy(c));
        HIP_TRY(up.wait_landed(c));
        bsg::PkeyArgs b = a;
        b.row_first = up.cuts[c]; b.row_end = up.cuts[c + 1];
        if (b.row_end == b.row_first) continue;
        const uint32_t grid = (b.row_end - b.row_first + bsg::kPkeyThreads - 1) / bsg::kPkeyThreads;
        HIP_TRY(timed([&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(bsg::k_partition_rows, dim3(grid), dim3(bsg::kPkeyThreads), 0, d.stream, e0, e1, 0, b, K.name);
        }));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    HIP_TRY(hipStreamSynchronize(d.copy_stream));
    // rounds: the claimed slots' texts join the dictionary (provisionally numbered), the rows still unassigned are resolved again
    std::vector<std::string> fresh;
    std::vector<uint32_t> fresh_row;
    std::vector<bsg::PkeyPending> pend(bsg::kPkeyPendingSlots);
    for (uint64_t round = 0;; ++round) {
        HIP_TRY(hipMemcpy(pend.data(), K.d_pending, pend.size() * sizeof(bsg::PkeyPending), hipMemcpyDeviceToHost));
        const size_t before = fresh.size();
        for (const bsg::PkeyPending &p : pend) {
            if (!p.tag) continue;
            std::string text;
            if (p.first_row >= n_rows || !keyed_host_text(K, rows + row_off[p.first_row], row_off[p.first_row + 1] - row_off[p.first_row], text))
                return fail(BSG_E_HIP, "keyed ingest: pending slot names row %u, which holds no decided text", p.first_row);
            fresh.push_back(std::move(text));
            fresh_row.push_back(p.first_row);
        }
        if (fresh.size() == before) break;
        if (round > n_rows) return fail(BSG_E_HIP, "keyed ingest: the partition rounds do not end");
        if ((uint64_t)I.n_sets + fresh.size() > BSG_PARTITION_MAX_SETS)
            return fail(BSG_E_INVALID, "keyed ingest: %u sets and %zu new keys exceed BSG_PARTITION_MAX_SETS (%u)", I.n_sets, fresh.size(), BSG_PARTITION_MAX_SETS);
        if (int32_t rc = keyed_upload(G, K, kc.hash_mask, fresh)) return rc;
        K.dirty = true;                        // until the sets below exist, the device's dictionary is this call's own
        HIP_TRY(hipMemcpyAsync(K.d_pending, unclaimed.data(), unclaimed.size() * sizeof(bsg::PkeyPending), hipMemcpyHostToDevice, d.stream));
        bsg::PkeyArgs b = a;
        b.dict = K.d_dict; b.pool = K.d_pool; b.dict_mask = K.dict_cap - 1;
        b.row_first = 0; b.row_end = n_rows;
        const uint32_t grid = (n_rows + bsg::kPkeyThreads - 1) / bsg::kPkeyThreads;
        HIP_TRY(timed([&](hipEvent_t e0, hipEvent_t e1) {
            hipExtLaunchKernelGGL(bsg::k_partition_assign, dim3(grid), dim3(bsg::kPkeyThreads), 0, d.stream, e0, e1, 0, b);
        }));
        HIP_TRY(hipStreamSynchronize(d.stream));
    }
    // the number of new keys is known: their sets, numbered by the lowest row that holds each
    const uint32_t n_new = (uint32_t)fresh.size(), old_sets = I.n_sets;
    std::vector<uint32_t> by_row(n_new), rank(n_new);
    std::iota(by_row.begin(), by_row.end(), 0u);
    std::sort(by_row.begin(), by_row.end(), [&](uint32_t x, uint32_t y) { return fresh_row[x] < fresh_row[y]; });
    for (uint32_t i = 0; i < n_new; ++i) rank[by_row[i]] = i;
    if (n_new) {
        if (int32_t rc = check_table_count((uint64_t)old_sets + n_new + I.n_parents)) return rc;
        const std::vector<uint32_t> parent(n_new, K.parent);
        if (int32_t rc = stream_add_sets(G, n_new, parent.data(), nullptr)) return rc;     // (K.dirty: the next call sends the dictionary of K.keys again)
        sync_sets(I, G);
        for (uint32_t i = 0; i < n_new; ++i) {
            K.set_of_key.emplace(fresh[by_row[i]], (uint32_t)K.keys.size());
            K.keys.push_back(fresh[by_row[i]]);
        }
    }
    if (K.dirty) if (int32_t rc = keyed_upload(G, K, kc.hash_mask, {})) return rc;
    sets.resize(n_rows);
    HIP_TRY(hipMemcpy(sets.data(), d_set, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    kept.clear(); kept_sets.clear();
    for (uint32_t r = 0; r < n_rows; ++r) {
        uint32_t s = sets[r];
        if (s == bsg::kPkeyNew) s = bsg::kPkeyUndecided;                        // (no round leaves one; handing it back is exact all the same)
        else if (s != bsg::kPkeyUndecided && (s & bsg::kPkeyProvisional)) s = old_sets + rank[s & ~bsg::kPkeyProvisional];
        if (s != bsg::kPkeyUndecided && s >= I.n_sets) return fail(BSG_E_HIP, "keyed ingest: row %u was given set %u of %u", r, s, I.n_sets);
        sets[r] = s;
        if (s != bsg::kPkeyUndecided) { kept.push_back(r); kept_sets.push_back(s); }
    }
    for (size_t i = 0; i + 1 < ev.v.size(); i += 2) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev.v[i], ev.v[i + 1]));
        *ms_partition += t;
    }
    memcpy(kc.out_set_of_row, sets.data(), (size_t)n_rows * 4);
    *kc.out_n_new_sets = n_new;
    return BSG_OK;
}

// One batch of a streaming ingest: rows in any order of sets, walked chunk by chunk in the order row_groups.hpp gives them.
// kc (bsg_ingest_append_rows_keyed; set_of_row is NULL): the batch is partitioned on the device first (partition_batch), then the rows
// it decided are walked from the resident bytes as one chunk; the rows it handed back join the fallback list and are not walked.
int32_t append_rows_stream(bsg_ctx *ctx, Ingest &I, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows, const uint32_t *set_of_row,
                           uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *n_fallback, const KeyedCall *kc = nullptr)
{
    IngestPart &G = *I.parts[0];
    Device &d = *G.dev;
    const char *call = kc ? "bsg_ingest_append_rows_keyed" : "bsg_ingest_append_rows";
    const LabTrace trace{call, d.id};
    d.calls.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    RowWalk w(ctx, G, trace, row_off, n_rows);
    uint32_t *d_order = nullptr, *d_set_of_order = nullptr;       // the walking order: this call's only, like the row bytes
    if (int32_t rc = w.buffers()) return rc;
    HIP_TRY(w.scratch.alloc(&d_order, (size_t)n_rows * 4));
    HIP_TRY(w.scratch.alloc(&d_set_of_order, (size_t)n_rows * 4));
    std::vector<uint32_t> part_sets, kept, kept_sets, fb;  // (keyed) every row's set, the rows to walk and their sets; the rows handed back
    float ms_partition = 0.f;
    uint32_t n_walk = n_rows;
    if (kc) {
        if (int32_t rc = partition_batch(ctx, I, G, w.scratch, rows, row_off, n_rows, w.d_rows, w.d_row_off, *kc, part_sets, kept, kept_sets, &ms_partition)) return rc;
        trace.lap("rows partitioned");
        set_of_row = kept_sets.data();
        n_walk = (uint32_t)kept.size();
        for (uint32_t r = 0; r < n_rows; ++r) if (part_sets[r] == bsg::kPkeyUndecided) fb.push_back(r);       // not walked: handed back here
        w.up.emplace(d, n_walk);           // the bytes are resident: positions [0, n_walk) of the walking order, one chunk
    } else w.up.emplace(d, rows, w.d_rows, row_off, n_rows, ctx->ingest_chunk_bytes);
    const bsg::RowsBySet by_set{d_order, d_set_of_order};
    std::vector<uint32_t> order(n_walk), set_of_order(n_walk), group_scratch;
    if (int32_t rc = w.walk(I.flags, I.tok_default ? nullptr : &I.spec, &by_set,
            [&](uint32_t rf, uint32_t re, hipStream_t cs) -> hipError_t {   // the chunk's walking order lands with its bytes
                bsh::group_rows_by_set(set_of_row, rf, re, G.n_sets, order.data(), set_of_order.data(), group_scratch);
                if (kc) for (uint32_t i = rf; i < re; ++i) order[i] = kept[order[i]];      // positions among the kept rows -> rows of the batch
                hipError_t e = hipMemcpyAsync(d_order + rf, order.data() + rf, (size_t)(re - rf) * 4, hipMemcpyHostToDevice, cs);
                if (e == hipSuccess) e = hipMemcpyAsync(d_set_of_order + rf, set_of_order.data() + rf, (size_t)(re - rf) * 4, hipMemcpyHostToDevice, cs);
                return e;
            }, fb)) return rc;
    if (kc) fb.erase(std::unique(fb.begin(), fb.end()), fb.end());      // (keyed: ascending, each row once, also without fields)
    const uint32_t nfb = (uint32_t)fb.size();
    {
        std::lock_guard<std::shared_mutex> lk2(ctx->mu);
        ctx->last_minmax_ms = G.ms_minmax;
        if (kc) ctx->last_partition_ms = ms_partition;
    }
    w.scratch.done();                      // both streams have been synchronised: the row bytes leave the device here
    *n_fallback = nfb;
    // a call that could not deliver its list is appended again (or walked on the host): its rows are counted by the call that does
    const bool count_only = !out_fallback_rows && fallback_cap == 0;
    if (!count_only && nfb > fallback_cap)
        return fail(BSG_E_INVALID, "%s: %u rows are handed back, out_fallback_rows has room for %u", call, nfb, fallback_cap);
    if (count_only && nfb) return BSG_OK;
    G.n_rows += n_rows;
    I.n_rows += n_rows;
    G.stats.n_rows += n_rows;
    G.stats.row_bytes += row_off[n_rows];
    G.stats.n_fallback_rows += nfb;
    if (nfb) memcpy(out_fallback_rows, fb.data(), (size_t)nfb * 4);
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_tokenizer_default(bsg_tokenizer *out)
{
    if (!out) return fail(BSG_E_INVALID, "null argument");
    *out = default_tokenizer();
    return BSG_OK;
}

int32_t bsg_ingest_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                        const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                        const uint32_t *slots_hint, uint32_t flags, uint64_t *out_ingest_id)
{
    BSG_ENTER(ctx);
    return ingest_rows_call(ctx, rows, row_off, n_rows, set_first_row, n_sets, parent_of_set, n_parents, slots_hint, flags, nullptr, out_ingest_id);
}

int32_t bsg_ingest_rows_tok(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                            const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                            const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id)
{
    BSG_ENTER(ctx);
    return ingest_rows_call(ctx, rows, row_off, n_rows, set_first_row, n_sets, parent_of_set, n_parents, slots_hint, flags, tok, out_ingest_id);
}

int32_t bsg_ingest_open(bsg_ctx *ctx, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents, const uint32_t *slots_hint,
                        uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id)
{
    BSG_ENTER(ctx);
    return ingest_open_call(ctx, n_sets, parent_of_set, n_parents, slots_hint, flags, tok, out_ingest_id);
}

int32_t bsg_ingest_rows_minmax(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                               const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                               const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id,
                               const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields)
{
    BSG_ENTER(ctx);
    bsg::MinMaxFields mm;
    if (int32_t rc = minmax_fields(field_bytes, field_off, n_fields, mm)) return rc;
    return ingest_rows_call(ctx, rows, row_off, n_rows, set_first_row, n_sets, parent_of_set, n_parents, slots_hint, flags, tok, out_ingest_id, &mm);
}

int32_t bsg_ingest_open_minmax(bsg_ctx *ctx, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents, const uint32_t *slots_hint,
                               uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id,
                               const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields)
{
    BSG_ENTER(ctx);
    bsg::MinMaxFields mm;
    if (int32_t rc = minmax_fields(field_bytes, field_off, n_fields, mm)) return rc;
    return ingest_open_call(ctx, n_sets, parent_of_set, n_parents, slots_hint, flags, tok, out_ingest_id, &mm);
}

int32_t bsg_ingest_minmax(bsg_ctx *ctx, uint64_t ingest_id, bsg_minmax *out, uint64_t cap)
{
    BSG_ENTER(ctx);
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    Ingest &I = *g;
    if (!I.has_mm) return fail(BSG_E_INVALID, "bsg_ingest_minmax: ingest %llu was made without MinMax fields", (unsigned long long)ingest_id);
    const uint32_t nf = I.mm_fields.n;
    const uint64_t need = (uint64_t)I.n_sets * nf;
    if (need && !out) return fail(BSG_E_INVALID, "null argument");
    if (need > cap) return fail(BSG_E_INVALID, "bsg_ingest_minmax: %llu records, out has room for %llu", (unsigned long long)need, (unsigned long long)cap);
    // every part owns its sets' records: the devices' partial results are folded by placing them
    for (auto &p : I.parts) {
        IngestPart &G = *p;
        if (!G.n_sets) continue;
        std::lock_guard<std::mutex> lk(G.dev->mu);
        if (int32_t rc = use_device(*G.dev)) return rc;
        if (!G.d_mm || G.n_sets > G.mm_cap || (uint64_t)G.set0 + G.n_sets > I.n_sets) return fail(BSG_E_INVALID, "bsg_ingest_minmax: the ingest holds no result");
        static_assert(sizeof(bsg_minmax) == sizeof(bsg::MinMaxRec), "bsg_minmax is the device record");
        HIP_TRY(hipStreamSynchronize(G.dev->stream));
        HIP_TRY(hipMemcpy(out + (size_t)G.set0 * nf, G.d_mm, (size_t)G.n_sets * nf * sizeof(bsg_minmax), hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < need; ++i) {
        out[i].reserved = 0;
        if (!out[i].present) out[i].min = out[i].max = 0;       // an absent index: the fold's neutral elements stay inside
        else out[i].present = 1;
    }
    return BSG_OK;
}

int32_t bsg_last_minmax_ms(bsg_ctx *ctx, float *minmax_ms)
{
    BSG_ENTER(ctx);
    if (!minmax_ms) return fail(BSG_E_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> lk(ctx->mu);
    *minmax_ms = ctx->last_minmax_ms;
    return BSG_OK;
}

int32_t bsg_ingest_add_sets(bsg_ctx *ctx, uint64_t ingest_id, uint32_t n_more, const uint32_t *parent_of_new_set,
                            const uint32_t *slots_hint_new, uint32_t *out_first_new_set)
{
    BSG_ENTER(ctx);
    if (!out_first_new_set) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_open_stream(ctx, ingest_id, g, "bsg_ingest_add_sets")) return rc;
    Ingest &I = *g;
    if (I.keyed) return fail(BSG_E_INVALID, "bsg_ingest_add_sets: ingest %llu is keyed, every set of it has a text (bsg_ingest_add_sets_keyed)", (unsigned long long)ingest_id);
    if (int32_t rc = check_table_count((uint64_t)I.n_sets + n_more + I.n_parents)) return rc;
    if (int32_t rc = check_parents(parent_of_new_set, n_more, I.n_parents)) return rc;
    *out_first_new_set = I.n_sets;
    if (n_more == 0) return BSG_OK;
    IngestPart &G = *I.parts[0];
    {
        std::lock_guard<std::mutex> lk(G.dev->mu);
        if (int32_t rc = use_device(*G.dev)) return rc;
        if (int32_t rc = stream_add_sets(G, n_more, parent_of_new_set, slots_hint_new)) return rc;
    }
    sync_sets(I, G);
    return BSG_OK;
}

int32_t bsg_ingest_append_rows(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                               const uint32_t *set_of_row, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    if (!out_n_fallback) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_open_stream(ctx, ingest_id, g, "bsg_ingest_append_rows")) return rc;
    *out_n_fallback = 0;
    if (n_rows == 0) return BSG_OK;
    if (!row_off || !set_of_row || (!out_fallback_rows && fallback_cap)) return fail(BSG_E_INVALID, "null argument");
    if (int32_t rc = refuse(bsh::check_rows(row_off, n_rows, rows != nullptr))) return rc;
    if (const uint32_t bad = bsh::first_bad_set(set_of_row, n_rows, g->n_sets); bad < n_rows)
        return fail(BSG_E_INVALID, "set_of_row[%u] = %u, the ingest has %u sets", bad, set_of_row[bad], g->n_sets);
    return append_rows_stream(ctx, *g, rows, row_off, n_rows, set_of_row, out_fallback_rows, fallback_cap, out_n_fallback);
}

// ---- keyed ingest: rows partitioned on the device by a top-level field (partition.hip.h) ----

int32_t bsg_ingest_open_keyed(bsg_ctx *ctx, uint32_t n_parents, uint32_t parent_of_new_sets, uint32_t flags, const bsg_tokenizer *tok,
                              uint64_t *out_ingest_id, const uint8_t *name_bytes, uint32_t name_len,
                              const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields)
{
    BSG_ENTER(ctx);
    if (name_len == 0) return fail(BSG_E_INVALID, "bsg_ingest_open_keyed: the partition field's name is empty");
    if (name_len > BSG_PARTITION_MAX_NAME) return fail(BSG_E_INVALID, "bsg_ingest_open_keyed: the partition field's name has %u bytes (at most %u)", name_len, BSG_PARTITION_MAX_NAME);
    if (!name_bytes) return fail(BSG_E_INVALID, "bsg_ingest_open_keyed: name_bytes is null");
    if (parent_of_new_sets != 0xFFFFFFFFu && parent_of_new_sets >= n_parents)
        return fail(BSG_E_INVALID, "bsg_ingest_open_keyed: parent_of_new_sets = %u, the ingest has %u parents", parent_of_new_sets, n_parents);
    bsg::MinMaxFields mm;
    if (n_fields || field_bytes || field_off) if (int32_t rc = minmax_fields(field_bytes, field_off, n_fields, mm)) return rc;
    auto K = std::make_unique<PartitionKeys>();
    memcpy(K->name.name, name_bytes, name_len);
    K->name.len = name_len;
    K->parent = parent_of_new_sets;
    return ingest_open_call(ctx, 0, nullptr, n_parents, nullptr, flags, tok, out_ingest_id, n_fields ? &mm : nullptr, std::move(K));
}

int32_t bsg_ingest_append_rows_keyed(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                     uint32_t *out_set_of_row, uint32_t *out_n_new_sets, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                     uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    if (!out_n_fallback || !out_n_new_sets) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_open_stream(ctx, ingest_id, g, "bsg_ingest_append_rows_keyed")) return rc;
    if (!g->keyed) return fail(BSG_E_INVALID, "bsg_ingest_append_rows_keyed: ingest %llu was not made by bsg_ingest_open_keyed", (unsigned long long)ingest_id);
    *out_n_fallback = 0;
    *out_n_new_sets = 0;
    if (n_rows == 0) return BSG_OK;
    if (!row_off || !out_set_of_row || (!out_fallback_rows && fallback_cap)) return fail(BSG_E_INVALID, "null argument");
    if (int32_t rc = refuse(bsh::check_rows(row_off, n_rows, rows != nullptr))) return rc;
    uint32_t mask = 0;
    { std::shared_lock<std::shared_mutex> lk(ctx->mu); mask = ctx->partition_hash_mask; }
    const KeyedCall kc{out_set_of_row, out_n_new_sets, mask};
    return append_rows_stream(ctx, *g, rows, row_off, n_rows, nullptr, out_fallback_rows, fallback_cap, out_n_fallback, &kc);
}

int32_t bsg_ingest_add_sets_keyed(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *key_bytes, const uint32_t *key_off, uint32_t n_keys,
                                  uint32_t *out_set_of_key)
{
    BSG_ENTER(ctx);
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_open_stream(ctx, ingest_id, g, "bsg_ingest_add_sets_keyed")) return rc;
    Ingest &I = *g;
    if (!I.keyed) return fail(BSG_E_INVALID, "bsg_ingest_add_sets_keyed: ingest %llu was not made by bsg_ingest_open_keyed", (unsigned long long)ingest_id);
    if (n_keys == 0) return BSG_OK;
    if (!key_off || !out_set_of_key) return fail(BSG_E_INVALID, "null argument");
    for (uint32_t i = 0; i < n_keys; ++i)
        if (key_off[i + 1] < key_off[i]) return fail(BSG_E_INVALID, "key_off not monotone at %u", i);
    if (key_off[n_keys] && !key_bytes) return fail(BSG_E_INVALID, "key_bytes is null");
    PartitionKeys &K = *I.keyed;
    // which texts are new is known before any set is made
    std::vector<std::string> fresh;
    std::unordered_map<std::string, uint32_t> fresh_set;
    for (uint32_t i = 0; i < n_keys; ++i) {
        std::string t(reinterpret_cast<const char *>(key_bytes) + key_off[i], key_off[i + 1] - key_off[i]);
        if (auto it = K.set_of_key.find(t); it != K.set_of_key.end()) { out_set_of_key[i] = it->second; continue; }
        auto [it, fresh_one] = fresh_set.emplace(t, I.n_sets + (uint32_t)fresh.size());
        if (fresh_one) fresh.push_back(std::move(t));
        out_set_of_key[i] = it->second;
    }
    if (fresh.empty()) return BSG_OK;
    if ((uint64_t)I.n_sets + fresh.size() > BSG_PARTITION_MAX_SETS)
        return fail(BSG_E_INVALID, "bsg_ingest_add_sets_keyed: %u sets and %zu new keys exceed BSG_PARTITION_MAX_SETS (%u)", I.n_sets, fresh.size(), BSG_PARTITION_MAX_SETS);
    if (int32_t rc = check_table_count((uint64_t)I.n_sets + fresh.size() + I.n_parents)) return rc;
    IngestPart &G = *I.parts[0];
    {
        std::lock_guard<std::mutex> lk(G.dev->mu);
        if (int32_t rc = use_device(*G.dev)) return rc;
        const std::vector<uint32_t> parent(fresh.size(), K.parent);
        if (int32_t rc = stream_add_sets(G, (uint32_t)fresh.size(), parent.data(), nullptr)) return rc;
    }
    sync_sets(I, G);
    for (std::string &t : fresh) {
        K.set_of_key.emplace(t, (uint32_t)K.keys.size());
        K.keys.push_back(std::move(t));
    }
    K.dirty = true;                            // the next keyed append sends the dictionary
    return BSG_OK;
}

int32_t bsg_ingest_keys(bsg_ctx *ctx, uint64_t ingest_id, uint32_t first, uint8_t *out_bytes, uint64_t bytes_cap, uint32_t *out_off,
                        uint32_t *out_n_keys, uint64_t *out_n_bytes)
{
    BSG_ENTER(ctx);
    if (!out_n_keys || !out_n_bytes) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    if (!g->keyed) return fail(BSG_E_INVALID, "bsg_ingest_keys: ingest %llu was not made by bsg_ingest_open_keyed", (unsigned long long)ingest_id);
    const PartitionKeys &K = *g->keyed;
    if (first > K.keys.size()) return fail(BSG_E_INVALID, "bsg_ingest_keys: first = %u, the ingest has %zu sets", first, K.keys.size());
    uint64_t total = 0;
    for (size_t s = first; s < K.keys.size(); ++s) total += K.keys[s].size();
    *out_n_keys = (uint32_t)(K.keys.size() - first);
    *out_n_bytes = total;
    if (!out_bytes && !out_off) return BSG_OK;       // the sizes only
    if (!out_off || (total && !out_bytes)) return fail(BSG_E_INVALID, "null argument");
    if (total > bytes_cap) return fail(BSG_E_INVALID, "bsg_ingest_keys: %llu bytes, out_bytes has room for %llu", (unsigned long long)total, (unsigned long long)bytes_cap);
    if (total > 0xFFFFFFFFull) return fail(BSG_E_INVALID, "bsg_ingest_keys: the texts exceed 32-bit offsets; ask for fewer sets");
    uint32_t at = 0;
    for (size_t s = first; s < K.keys.size(); ++s) {
        out_off[s - first] = at;
        if (!K.keys[s].empty()) memcpy(out_bytes + at, K.keys[s].data(), K.keys[s].size());
        at += (uint32_t)K.keys[s].size();
    }
    out_off[K.keys.size() - first] = at;
    return BSG_OK;
}

int32_t bsg_last_partition_ms(bsg_ctx *ctx, float *partition_ms)
{
    BSG_ENTER(ctx);
    if (!partition_ms) return fail(BSG_E_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> lk(ctx->mu);
    *partition_ms = ctx->last_partition_ms;
    return BSG_OK;
}

int32_t bsg_ingest_fallback_rows(bsg_ctx *ctx, uint64_t ingest_id, uint32_t *rows_out, uint32_t cap, uint32_t *n_out)
{
    BSG_ENTER(ctx);
    if (!ctx || !n_out) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    if (g->streaming) return fail(BSG_E_INVALID, "a streaming ingest hands its rows back batch by batch: bsg_ingest_append_rows returns them");
    *n_out = (uint32_t)g->fallback.size();
    if (rows_out) memcpy(rows_out, g->fallback.data(), (size_t)std::min<uint32_t>(cap, *n_out) * 4);
    return BSG_OK;
}

int32_t bsg_ingest_add_entries(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *bytes, const uint32_t *offsets, uint32_t n_entries,
                               const uint32_t *set_of_entry, const uint32_t *kind_of_entry)
{
    BSG_ENTER(ctx);
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    if (g->finished) return fail(BSG_E_INVALID, "ingest already finished");
    if (n_entries == 0) return BSG_OK;
    if (!offsets || !set_of_entry || !kind_of_entry) return fail(BSG_E_INVALID, "null argument");
    for (uint32_t e = 0; e < n_entries; ++e) {
        if (offsets[e + 1] < offsets[e]) return fail(BSG_E_INVALID, "offsets not monotone at %u", e);
        if (set_of_entry[e] >= g->n_sets || kind_of_entry[e] > 2) return fail(BSG_E_INVALID, "entry %u: set or kind out of range", e);
    }
    if (offsets[n_entries] && !bytes) return fail(BSG_E_INVALID, "bytes is null");
    // every entry goes to the part that owns its set (repacked per part; the host walker's entries are few)
    const uint32_t np = (uint32_t)g->parts.size();
    std::vector<std::vector<uint8_t>> pbytes(np);
    std::vector<std::vector<uint32_t>> poff(np, std::vector<uint32_t>{0}), ptab(np);
    for (uint32_t e = 0; e < n_entries; ++e) {
        const uint32_t q = np == 1 ? 0 : g->part_of_set(set_of_entry[e]);
        pbytes[q].insert(pbytes[q].end(), bytes + offsets[e], bytes + offsets[e + 1]);
        poff[q].push_back((uint32_t)pbytes[q].size());
        ptab[q].push_back((set_of_entry[e] - g->parts[q]->set0) * 3 + kind_of_entry[e]);
    }
    return run_parts(np, [&](uint32_t q) -> int32_t {
        const uint32_t n = (uint32_t)ptab[q].size();
        if (!n) return BSG_OK;
        IngestPart &G = *g->parts[q];
        Device &d = *G.dev;
        std::lock_guard<std::mutex> lk(d.mu);
        if (int32_t rc = use_device(d)) return rc;
        const uint32_t n_bytes = poff[q][n];
        HIP_TRY(d.stage_a.reserve((size_t)n_bytes + 64));
        HIP_TRY(d.stage_off.reserve((size_t)n + 1));
        HIP_TRY(d.stage_fstart.reserve(n));
        if (n_bytes) HIP_TRY(hipMemcpyAsync(d.stage_a.p, pbytes[q].data(), n_bytes, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d.stage_off.p, poff[q].data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d.stage_fstart.p, ptab[q].data(), (size_t)n * 4, hipMemcpyHostToDevice, d.stream));
        float ms = 0.f;
        return run_until_fits(G, 0, G.n_sets * 3, &ms, [&](hipEvent_t e0, hipEvent_t e1) -> int32_t {
            hipExtLaunchKernelGGL(bsg::k_ingest_add, dim3((n + 255) / 256), dim3(256), 0, d.stream, e0, e1, 0,
                                  d.stage_a.p, d.stage_off.p, d.stage_fstart.p, n, G.d_tables, G.d_counts, G.d_status, ctx->fp_key);
            return BSG_OK;
        });
    });
}

int32_t bsg_ingest_finish(bsg_ctx *ctx, uint64_t ingest_id, uint64_t *out_counts, uint32_t *out_status)
{
    BSG_ENTER(ctx);
    if (!ctx || !out_counts) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    Ingest &I = *g;
    if (!I.finished) {
        const uint32_t np = (uint32_t)I.parts.size();
        if (int32_t rc = run_parts(np, [&](uint32_t q) -> int32_t { return finish_part(ctx, *I.parts[q]); })) return rc;
        if (np > 1 && I.n_parents) if (int32_t rc = merge_parents(ctx, I)) return rc;
        I.counts.assign(I.n_tables(), 0);
        I.status.assign(I.n_tables(), 0);
        for (auto &p : I.parts)
            for (uint32_t t = 0; t < p->n_sets * 3; ++t) {
                I.counts[(size_t)p->set0 * 3 + t] = p->counts[t];
                I.status[(size_t)p->set0 * 3 + t] = p->status[t];
            }
        const IngestPart &PP = I.merged ? *I.merged : *I.parts[0];
        const uint32_t pbase = I.merged ? 0 : PP.n_sets * 3;
        for (uint32_t t = 0; t < I.n_parents * 3; ++t) {
            I.counts[(size_t)I.n_sets * 3 + t] = PP.counts[pbase + t];
            I.status[(size_t)I.n_sets * 3 + t] = PP.status[pbase + t];
        }
        I.finished = true;
    }
    for (uint32_t t = 0; t < I.n_tables(); ++t) out_counts[t] = I.counts[t];
    if (out_status) {
        for (uint32_t s = 0; s < I.n_sets + I.n_parents; ++s)
            out_status[s] = std::max({I.status[s * 3], I.status[s * 3 + 1], I.status[s * 3 + 2]});
        // a set that cannot be represented leaves its file-level union incomplete as well
        for (uint32_t s = 0; s < I.n_sets; ++s)
            if (I.parent_of_set[s] != 0xFFFFFFFFu) out_status[I.n_sets + I.parent_of_set[s]] = std::max(out_status[I.n_sets + I.parent_of_set[s]], out_status[s]);
    }
    return BSG_OK;
}

}  // extern "C"

namespace {

// ---- resident arenas straight from the words the parts have just built ----
// Block b of an arena lives on device b % n like in every other arena.  The shards are laid out and allocated BEFORE the
// parts build (the geometry is known from the descriptors); every part then copies the blocks it built — its three filters
// sit back to back in the part's word buffer — into their shards, device to device (peer copies), behind its own build and
// under its own device lock (the part's word buffer is the device's shared staging).
struct ArenaPlan {
    std::shared_ptr<Arena> arena;
    std::vector<uint64_t> dst_off;            // block -> word offset of its span inside its shard
    uint64_t *out_id = nullptr;
};

int32_t plan_arena(bsg_ctx *ctx, const bsg_filter_desc *desc, uint32_t n_blocks, ArenaPlan &plan)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    plan.arena = std::make_shared<Arena>();
    plan.arena->n_blocks = n_blocks;
    plan.arena->shards.resize(nd);
    plan.dst_off.assign(n_blocks, 0);
    hipError_t e = hipSuccess;
    for (uint32_t di = 0; di < nd && e == hipSuccess; ++di) {
        ArenaShard &s = plan.arena->shards[di];
        const bsh::ShardLayout L = bsh::layout_shard(desc, n_blocks, di, nd);
        static_cast<bsh::ShardStats &>(s) = L.stats;
        s.n_blocks = L.n_blocks;
        s.n_words = L.n_words;
        for (uint32_t lb = 0; lb < L.n_blocks; ++lb) plan.dst_off[lb * nd + di] = L.block_off[lb];
        std::vector<DevDesc> dd(L.filters.size());
        std::transform(L.filters.begin(), L.filters.end(), dd.begin(), dev_desc);
        const uint64_t cursor = L.n_words - kAlignWords;
        e = hipSetDevice(ctx->devs[di]->id);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_words), s.n_words * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s.d_desc), std::max<size_t>(dd.size(), 1) * sizeof(DevDesc));
        if (e == hipSuccess) e = hipMemset(s.d_words + cursor, 0, kAlignWords * 8);
        if (e == hipSuccess && !dd.empty()) e = hipMemcpy(s.d_desc, dd.data(), dd.size() * sizeof(DevDesc), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        free_arena(ctx, *plan.arena);
        plan.arena.reset();
        return fail(e == hipErrorOutOfMemory ? BSG_E_NOMEM : BSG_E_HIP, "resident arena: %s", hipGetErrorString(e));
    }
    return BSG_OK;
}

// copies blocks [b0, b1) of the plan's arena out of d_words (layout `local`: descriptor i = block b0 + i / 3, word offsets into
// d_words) on device d, whose lock the caller holds and whose stream the copies are enqueued on
int32_t fill_arena(bsg_ctx *ctx, Device &d, const uint64_t *d_words, const bsg_filter_desc *local, uint32_t b0, uint32_t b1, const ArenaPlan &plan)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    struct Span { uint32_t di; uint64_t src, dst, words; };
    std::vector<Span> spans;
    for (uint32_t b = b0; b < b1; ++b) {
        const bsg_filter_desc *d3 = local + (size_t)(b - b0) * 3;
        uint64_t lo = ~0ull;
        for (uint32_t c = 0; c < 3; ++c) if (d3[c].m) lo = std::min(lo, d3[c].word_off);
        if (lo == ~0ull) continue;
        const uint64_t words = bsh::block_span_words(d3);
        const uint32_t di = b % nd;
        if (!spans.empty() && spans.back().di == di && spans.back().src + spans.back().words == lo && spans.back().dst + spans.back().words == plan.dst_off[b])
            spans.back().words += words;                              // (one device: neighbouring blocks merge into one copy)
        else
            spans.push_back(Span{di, lo, plan.dst_off[b], words});
    }
    for (const Span &sp : spans) {
        const ArenaShard &s = plan.arena->shards[sp.di];
        // (a block's last span may reach past the words the build wrote: the build buffer is padded to the alignment too)
        HIP_TRY(peer_copy(ctx, sp.di, s.d_words + sp.dst, dev_index(ctx, &d), d_words + sp.src, sp.words * 8, d.stream));
    }
    HIP_TRY(hipStreamSynchronize(d.stream));
    return BSG_OK;
}

// What one part contributes to a build: tables [t0, t1) of part G are the caller's tables [i0, i1).
struct PartBuild : BuildPart {
    IngestPart *G = nullptr;
    uint32_t t0 = 0, t1 = 0;
    PartBuild(IngestPart *g, uint32_t t1_, uint32_t i0_) : G(g), t1(t1_) { i0 = i0_; i1 = i0_ + t1_; }
};

int32_t build_part(bsg_ctx *ctx, PartBuild &B, const bsg_filter_desc *desc_in, uint64_t *out_words, const SectionsOut *sections,
                   const ArenaPlan *sets_plan, const ArenaPlan *parents_plan, uint32_t n_sets_global)
{
    IngestPart &G = *B.G;
    const uint32_t nt = B.t1 - B.t0;
    if (nt == 0) return BSG_OK;
    // the part's descriptors: word offsets relative to the part (words route) or a layout of its own (sections route: every
    // filter on a 128-byte boundary, so a run of blocks becomes a resident arena with plain copies)
    std::vector<bsg_filter_desc> local(desc_in + B.i0, desc_in + B.i1);
    uint64_t n_words = 2;
    if (sections) {
        uint64_t cursor = 0;
        for (bsg_filter_desc &f : local) { f.word_off = cursor; cursor += bsh::aligned_words(f.m); }
        n_words = std::max<uint64_t>(cursor, 2);
    } else {
        for (bsg_filter_desc &f : local) if (f.m) f.word_off -= B.w_lo;
        n_words = std::max<uint64_t>(B.w_hi - B.w_lo, 2);
    }
    // a staged bitset sits beside k_build_sets' compaction list in LDS; a sliced table is cut by slots, four per entry of a slice
    PartWork<bsg::SetBuildItem> W = classify_part<bsg::SetBuildItem>(ctx, local, bsg::kSetListBytes, [&](uint32_t i) { return G.counts[B.t0 + i]; },
        [&](std::vector<bsg::SetBuildItem> &items, uint32_t i, bool staged) {
            const uint32_t t = B.t0 + i;
            const uint64_t cap = (uint64_t)G.tables[t].mask + 1, slice = (uint64_t)kBuildSliceEntries * 4;
            if (staged) { items.push_back({t, 1u, 0, cap}); return; }
            for (uint64_t s = 0; s < cap; s += slice) items.push_back({t, 0u, s, std::min(cap, s + slice)});
        });
    const std::vector<bsg::SetBuildItem> &items = W.items;
    Device &d = *G.dev;
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    HIP_TRY(d.stage_words.reserve(n_words));
    HIP_TRY(hipMemsetAsync(d.stage_words.p, 0, n_words * 8, d.stream));
    if (!items.empty() || !W.binned.empty()) {
        HIP_TRY(d.stage_desc.reserve(nt));
        HIP_TRY(hipMemcpyAsync(d.stage_desc.p, W.dd.data(), W.dd.size() * sizeof(DevDesc), hipMemcpyHostToDevice, d.stream));
        Scratch scratch(d);
        bsg::SetBuildItem *d_items = nullptr;
        HIP_TRY(scratch.alloc(&d_items, std::max<size_t>(items.size(), 1) * sizeof(bsg::SetBuildItem)));
        EventList ev;
        HIP_TRY(ev.add(2));
        if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::SetBuildItem), hipMemcpyHostToDevice, d.stream));
        DispatchSpan span{ev.v[0], ev.v[1]};
        if (!items.empty()) {
            // items name the part's own table indices; the descriptor array holds tables [t0, t1) only: its base moves back by t0
            bsg::SetBuildArgs a{G.d_tables, d_items, d.stage_desc.p - B.t0, d.stage_words.p};
            hipExtLaunchKernelGGL(bsg::k_build_sets, dim3((uint32_t)items.size()), dim3(bsg::kBuildSetsThreads), (uint32_t)W.lds_bytes(), d.stream,
                                  span.first(), span.last(W.binned.empty()), 0, a);
            HIP_TRY(hipGetLastError());
        }
        uint32_t *d_over = nullptr;
        if (int32_t rc = enqueue_binned_filters(d, W.dd, W.binned, false, scratch, span, &d_over, [&](uint32_t i, bsg::BinArgs &a) -> int32_t {
                const uint32_t t = B.t0 + i;
                a.t = G.tables[t];
                a.n_slots = (uint64_t)G.tables[t].mask + 1;
                a.n_locs_cap = (uint32_t)((uint64_t)G.counts[t] * local[i].k);
                return BSG_OK;
            })) return rc;
        HIP_TRY(hipStreamSynchronize(d.stream));
        scratch.done();
        (void)hipEventElapsedTime(&B.ms, ev.v[0], ev.v[1]);
        // n_locs_cap comes from the counts bsg_ingest_finish read, and entries may have joined the tables since: the binning passes
        // flag what did not fit, and the call fails on it.  (The entries route counts exactly and has nothing to read.)
        if (d_over) {
            uint32_t over = 0;
            HIP_TRY(hipMemcpy(&over, d_over, 4, hipMemcpyDeviceToHost));
            if (over) return fail(BSG_E_INVALID, "a set holds more entries than bsg_ingest_finish counted");
        }
    }
    if (int32_t rc = deliver_part(d, B, local, out_words, sections)) return rc;
    if (sections) {
        // the caller's tables [i0, i1) are blocks i0 / 3 ...: sets first, parents after
        const uint32_t blk0 = B.i0 / 3, blk1 = blk0 + nt / 3;
        if (sets_plan && blk0 < n_sets_global) {
            const uint32_t e1 = std::min(blk1, n_sets_global);
            if (int32_t rc = fill_arena(ctx, d, d.stage_words.p, local.data(), blk0, e1, *sets_plan)) return rc;
        }
        if (parents_plan && blk1 > n_sets_global) {
            const uint32_t s0 = std::max(blk0, n_sets_global);
            if (int32_t rc = fill_arena(ctx, d, d.stage_words.p, local.data() + (size_t)(s0 - blk0) * 3, s0 - n_sets_global, blk1 - n_sets_global, *parents_plan)) return rc;
        }
    }
    return BSG_OK;
}

int32_t ingest_build_common(bsg_ctx *ctx, uint64_t ingest_id, const bsg_filter_desc *desc, uint64_t *out_words, uint64_t n_words,
                            const SectionsOut *sections, uint64_t *out_sets_arena = nullptr, uint64_t *out_parents_arena = nullptr)
{
    BSG_ENTER(ctx);
    if (!ctx || !desc || (!out_words && !sections)) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    Ingest &I = *g;
    if (!I.finished) return fail(BSG_E_INVALID, "bsg_ingest_finish has not run");
    const uint32_t nt = I.n_tables();
    if (!sections) if (int32_t rc = validate_descs(desc, nt, n_words)) return rc;
    if (sections)
        for (uint32_t t = 0; t < nt; ++t)
            if (desc[t].m && (desc[t].k == 0 || desc[t].k > kMaxHashCount)) return fail(BSG_E_INVALID, "descriptor %u: k = %u outside [1, %llu]", t, desc[t].k, (unsigned long long)kMaxHashCount);
    // ---- who builds what: every part its sets; the parents by the merged part (several parts) or by the only part ----
    std::vector<PartBuild> jobs;
    if (I.parts.size() == 1) {
        jobs.emplace_back(I.parts[0].get(), I.parts[0]->n_tables(), 0u);       // sets and parents in one go
    } else {
        for (auto &p : I.parts) jobs.emplace_back(p.get(), p->n_sets * 3, p->set0 * 3);
        if (I.merged) jobs.emplace_back(I.merged.get(), I.n_parents * 3, I.n_sets * 3);
    }
    // words route: a job owns the words [first filter, end of last filter) of the caller's arena: the layout must ascend
    // with the table index, or the jobs' copies back would overlap
    if (!sections && jobs.size() > 1 && !bsh::offsets_ascend(desc, nt))
        return fail(BSG_E_UNSUPPORTED, "an ingest cut over %zu devices needs filter word offsets that ascend with the table index", jobs.size());
    if (int32_t rc = check_region(bsh::plan_parts(desc, jobs, n_words, sections != nullptr), sections)) return rc;
    if (!sections && jobs.size() > 1) bsh::zero_unowned(out_words, n_words, jobs);
    ArenaPlan sets_plan, parents_plan;
    if (sections && out_sets_arena) { *out_sets_arena = 0; if (int32_t rc = plan_arena(ctx, desc, I.n_sets, sets_plan)) return rc; }
    if (sections && out_parents_arena) {
        *out_parents_arena = 0;
        if (int32_t rc = plan_arena(ctx, desc + (size_t)I.n_sets * 3, I.n_parents, parents_plan)) {
            if (sets_plan.arena) free_arena(ctx, *sets_plan.arena);
            return rc;
        }
    }
    const int32_t rc = run_parts((uint32_t)jobs.size(), [&](uint32_t i) -> int32_t {
        return build_part(ctx, jobs[i], desc, out_words, sections, sets_plan.arena ? &sets_plan : nullptr, parents_plan.arena ? &parents_plan : nullptr, I.n_sets);
    });
    if (rc) {
        if (sets_plan.arena) free_arena(ctx, *sets_plan.arena);
        if (parents_plan.arena) free_arena(ctx, *parents_plan.arena);
        return rc;
    }
    fold_parts(jobs, sections, I.ms_build, I.ms_encode);
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        if (sections) ctx->last_encode_ms = I.ms_encode;
        if (sets_plan.arena) { const uint64_t id = ctx->next_id++; ctx->arenas[id] = sets_plan.arena; *out_sets_arena = id; }
        if (parents_plan.arena) { const uint64_t id = ctx->next_id++; ctx->arenas[id] = parents_plan.arena; *out_parents_arena = id; }
    }
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_ingest_build(bsg_ctx *ctx, uint64_t ingest_id, const bsg_filter_desc *desc, uint64_t *out_words, uint64_t n_words)
{
    if (!out_words) return fail(BSG_E_INVALID, "null argument");
    return ingest_build_common(ctx, ingest_id, desc, out_words, n_words, nullptr);
}

int32_t bsg_ingest_build_sections(bsg_ctx *ctx, uint64_t ingest_id, const bsg_filter_desc *desc, uint8_t *out_region,
                                  uint64_t region_cap, uint64_t *out_sec_off, uint64_t *out_sets_arena_id,
                                  uint64_t *out_parents_arena_id)
{
    if (!out_region || !out_sec_off) return fail(BSG_E_INVALID, "null argument");
    SectionsOut so{out_region, region_cap, out_sec_off};
    return ingest_build_common(ctx, ingest_id, desc, nullptr, 0, &so, out_sets_arena_id, out_parents_arena_id);
}

int32_t bsg_ingest_stats_read(bsg_ctx *ctx, uint64_t ingest_id, bsg_ingest_stats *out)
{
    BSG_ENTER(ctx);
    if (!ctx || !out) return fail(BSG_E_INVALID, "null argument");
    std::shared_ptr<Ingest> g;
    if (int32_t rc = get_ingest(ctx, ingest_id, g)) return rc;
    // device times: the slowest part (the parts run side by side); volumes: the sum
    bsg_ingest_stats st{};
    uint64_t bytes = 0;
    for (auto &p : g->parts) {
        st.n_rows += p->stats.n_rows;
        st.table_grows += p->stats.table_grows;
        st.row_bytes += p->stats.row_bytes;
        st.ms_walk = std::max(st.ms_walk, p->stats.ms_walk);
        st.ms_union = std::max(st.ms_union, p->stats.ms_union);
        bytes += p->slot_bytes;
    }
    if (g->merged) bytes += g->merged->slot_bytes;
    st.n_fallback_rows = g->streaming ? g->parts[0]->stats.n_fallback_rows : (uint32_t)g->fallback.size();   // (a stream: summed over the appends)
    st.ms_union += g->ms_merge;
    st.ms_build = g->ms_build;
    st.ms_encode = g->ms_encode;
    st.table_bytes = bytes;
    *out = st;
    return BSG_OK;
}

int32_t bsg_ingest_free(bsg_ctx *ctx, uint64_t ingest_id)
{
    BSG_ENTER(ctx);
    if (!ctx) return fail(BSG_E_INVALID, "ctx is null");
    std::shared_ptr<Ingest> g;
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        auto it = ctx->ingests.find(ingest_id);
        if (it == ctx->ingests.end()) return fail(BSG_E_NOTFOUND, "unknown ingest id %llu", (unsigned long long)ingest_id);
        g = it->second;
        ctx->ingests.erase(it);
    }
    free_ingest(*g);
    return BSG_OK;
}

}  // extern "C"
