/*
 * bloomgpu.h — C-ABI of libbloomgpu.so: bloomsearch's hierarchical bloom-filter
 * construct + probe hot path on AMD MI355X (gfx950 / CDNA4).
 *
 * This is the drop-in boundary.  The reference (github.com/danthegoodman1/bloomsearch,
 * pure Go) has no plugin seam at the bloom level, so the Go host binds these entry
 * points with cgo at exactly the internal seams named beside each function
 * (see INTEGRATION.md for the cgo stub).  Everything here is plain C99: int32
 * status returns, opaque context, caller-owned pointers that are only read or
 * written for the duration of the call (cgo rule: C never retains a Go pointer).
 *
 * Semantics replaced (reference file:line):
 *   bsg_hash_entries / bsg_build ... buildSizedBloomFilter's AddString loop, ingest.go:139-145
 *                                    (bloom/v3 v3.7.0 baseHashes + location + bitset.Set)
 *   bsg_arena_load ................. the decoded result of blockFilterCursor.filtersFor /
 *                                    parseFilterSection for every block, file_format.go:392-448,575
 *   bsg_batch_create ............... the pruneBloomQuery tree, query_exec.go:220 / query.go:586-718,
 *                                    with each distinct term hashed ONCE instead of per TestString
 *   bsg_probe / bsg_probe_batch .... evaluateBlockFilters' per-block loop + evaluateBloomFilters /
 *                                    evaluateBloomExpression / evaluateBloomCondition,
 *                                    query_exec.go:572-615 and :75-159
 *   bsg_or_reduce .................. north-star extension (fixed-geometry OR of block filters into a
 *                                    file-level filter); the reference rebuilds instead, merge.go:447-453
 *
 * Threading: every entry point is re-entrant on one context (internal mutex
 * around handle tables, per-call stream ordering); no thread-local "current
 * device" is assumed.  No callbacks, no exceptions cross the boundary.
 */
#ifndef BLOOMGPU_H
#define BLOOMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSG_API __attribute__((visibility("default")))

/* ---- status codes ---- */
#define BSG_OK              0
#define BSG_E_INVALID      -1  /* bad argument / malformed descriptor or program (rejected before any launch) */
#define BSG_E_HIP          -2  /* HIP runtime error (message in bsg_last_error) */
#define BSG_E_NOMEM        -3
#define BSG_E_NOTFOUND     -4  /* unknown arena / batch id */
#define BSG_E_UNSUPPORTED  -5
#define BSG_E_NODEVICE     -6  /* no gfx950 device visible: the library never falls back to a CPU path */

/* ---- filter kinds: which of a block's three filters a term tests
 *      (BloomField / BloomToken / BloomFieldToken, query.go:480-484) ---- */
#define BSG_KIND_FIELD        0u
#define BSG_KIND_TOKEN        1u
#define BSG_KIND_FIELD_TOKEN  2u
#define BSG_KIND_FIELD_REGEX  3u   /* row matcher only (bsg_match_rows_regex): entry 2i = field, 2i + 1 = pattern */
#define BSG_KIND_SUBSTRING        4u   /* bsg_match_rows_substr / _many_substr / _regex_substr / _many_regex_substr only: entry 2i empty, 2i + 1 = the needle */
#define BSG_KIND_FIELD_SUBSTRING  5u   /* ... entry 2i = the field, 2i + 1 = the needle */
#define BSG_KIND_FIELD_RANGE      6u   /* bsg_match_rows_range / _many_range / _wide_range(_rows) / _regex_substr_range / _many_regex_substr_range only: entry 2i = the field, 2i + 1 = lo, hi, flags ("Range conditions") */
#define BSG_RANGE_ENTRY_BYTES 17u      /* lo (int64, little-endian), hi (the same), one byte of BSG_RANGE_* */
#define BSG_RANGE_NO_LO   1u           /* no lower bound (lo is ignored) */
#define BSG_RANGE_NO_HI   2u           /* no upper bound (hi is ignored) */
#define BSG_RANGE_LO_OPEN 4u           /* value > lo instead of value >= lo */
#define BSG_RANGE_HI_OPEN 8u           /* value < hi instead of value <= hi */

/* ---- query program opcodes: op = (opcode << 28) | arg, postfix order ----
 * TERM i : push TestString(term i) against the block's filter of term i's kind;
 *          absent filter => true (fail-open, query_exec.go:137-151)
 * AND n  : pop n, push conjunction   (n == 0 => true,  query_exec.go:115-121)
 * OR  n  : pop n, push disjunction   (n == 0 => false, query_exec.go:105-114)
 * TRUE   : nil expression / nil condition           (query_exec.go:84,97)
 * FALSE  : unknown expression or condition type     (query_exec.go:122,156)
 * A query with zero ops is a nil BloomQuery => true (query_exec.go:81-83). */
#define BSG_OP_TERM   0u
#define BSG_OP_AND    1u
#define BSG_OP_OR     2u
#define BSG_OP_TRUE   3u
#define BSG_OP_FALSE  4u
#define BSG_OP(opcode, arg) (((uint32_t)(opcode) << 28) | ((uint32_t)(arg) & 0x0FFFFFFFu))

/* One distinct query term: the four bloom/v3 base hashes of the probed string
 * (Field, Token, or Field+"::"+Token — tokenizer.go:509-511) and the filter kind. */
typedef struct bsg_term {
    uint64_t h[4];
    uint32_t kind;
    uint32_t reserved;
} bsg_term;

/* One filter inside a word arena.  Bit i of the filter is bit (i & 63) of
 * words[word_off + (i >> 6)] (bitset v1.10.0 layout; native little-endian u64,
 * i.e. the Go []uint64 as-is — the big-endian swap of WriteTo/ReadFrom is the
 * wire format only).  m == 0 marks an absent (nil) filter. */
typedef struct bsg_filter_desc {
    uint64_t word_off;
    uint64_t m;
    uint32_t k;
    uint32_t reserved;
} bsg_filter_desc;

/* Device-side timing of probes issued with BSG_PROBE_TIMED (HIP events on the
 * library's own stream; accumulated until read). */
typedef struct bsg_timing {
    uint64_t n_probes;           /* timestamped k_probe_terms / k_probe_gather dispatches                    */
    double   ms_terms_kernel;    /* sum of their durations (the HBM stream)                                 */
    double   ms_eval_kernel;     /* sum of the timestamped k_eval_programs durations (n_eval of them)       */
    uint64_t stream_bytes;       /* bitset bytes those dispatches move: every referenced bitset once where the launch streams
                                    (k_probe_terms); where it gathers (k_probe_gather), the 128-byte lines the bit tests it EXECUTED
                                    (counted on the device: a term absent from a block stops early) are expected to touch,
                                    lines x (1 - exp(-tests / lines)) per filter — what the counters show */
    uint64_t n_probe_arenas;     /* arenas those dispatches covered (one dispatch probes a group of arenas) */
    uint64_t n_eval;
    uint64_t n_fused;            /* timestamped k_probe_fused dispatches (probe of group i + eval of i-1)   */
    double   ms_fused_kernel;
    uint64_t fused_stream_bytes; /* bitset bytes streamed by their probe role                               */
    uint64_t n_fused_arenas;
    uint64_t n_folded;           /* timestamped k_probe_eval dispatches (probe + per-tile program evaluation in one) */
    double   ms_folded_kernel;
    uint64_t folded_stream_bytes;/* bitset bytes streamed by them                                           */
    uint64_t n_folded_arenas;
} bsg_timing;

#define BSG_PROBE_ASYNC  1u  /* enqueue only; caller later calls bsg_sync                    */
#define BSG_PROBE_TIMED  2u  /* timestamp the dispatches (see bsg_timing_read)               */
#define BSG_PROBE_NOFUSE 4u  /* never fuse or fold: every group runs as k_probe_terms + k_eval_programs */
#define BSG_PROBE_ROWS_PACKED 8u /* bsg_probe_many_rows only: LIST / DENSE payloads packed per run of 256 queries (below)    */

typedef struct bsg_ctx bsg_ctx;

/* ---- lifecycle (engine construct / Stop) ---- */
BSG_API int32_t bsg_device_count(void);
/* out_matrix[i * n + j] (n = the context's devices) = 1 when device i reaches device j's memory directly (peer access over xGMI
 * enabled at bsg_open, or the same device), 0 when copies between the two are staged through host memory by the runtime:
 * still correct, at PCIe speed, and announced on stderr once per pair (BSG_QUIET=1 silences it). */
BSG_API int32_t bsg_peer_access(bsg_ctx *ctx, uint8_t *out_matrix, uint32_t n);
BSG_API int32_t bsg_open(const int32_t *device_ids, int32_t n_devices, bsg_ctx **out_ctx);
BSG_API int32_t bsg_close(bsg_ctx *ctx);
/* ---- errors ----
 * Every failing call records its message on the handle it was made on; bsg_last_error(handle) returns a private copy of
 * it (valid until the calling thread's next bsg_last_error) and may run on ANY OS thread — nothing here depends on the
 * caller staying on one thread between the failing call and the read (a goroutine may migrate between two cgo calls,
 * SURVEY 7 hard part 6: no runtime.LockOSThread).  A context shared by concurrent callers has ONE slot, so a Go host
 * gives every goroutine-confined caller (flush worker, merge, each query's file worker) a SCOPE of its own:
 * bsg_scope_open returns a lightweight alias of the context — valid wherever a bsg_ctx* is — that owns nothing but its
 * own error slot; close it with bsg_close before the context.  bsg_last_error(NULL) serves only the context-free entry
 * points (bsg_open, bsg_estimate_parameters, bsg_sections_size) and is thread-local; bsg_open_err returns bsg_open's
 * message in the same call instead. */
BSG_API const char *bsg_last_error(bsg_ctx *ctx);
BSG_API int32_t bsg_last_error_copy(bsg_ctx *ctx, char *buf, uint64_t cap);
BSG_API int32_t bsg_scope_open(bsg_ctx *ctx, bsg_ctx **out_scope);
BSG_API int32_t bsg_open_err(const int32_t *device_ids, int32_t n_devices, bsg_ctx **out_ctx, char *errbuf, uint64_t cap);
BSG_API int32_t bsg_sync(bsg_ctx *ctx);

/* Construct / match work on a context over several devices (bsg_hash_entries, bsg_build*, bsg_ingest_*, bsg_match_rows): a call
 * large enough is cut into one part per device — contiguous runs of entries / filters / sets / rows, each on a thread of its
 * own (partitions are independent in flush.go:191-254, surviving blocks in query_exec.go:729-764) — and a smaller call takes ONE
 * device, chosen round-robin among those nobody holds, so the flush worker, a merge and concurrent queries' block workers
 * land on different GPUs.  Results do not depend on the number of devices.  out_calls[i]: parts device i has served so far. */
BSG_API int32_t bsg_device_calls(bsg_ctx *ctx, uint64_t *out_calls, uint32_t cap);

/* ---- sizing: bloom/v3 EstimateParameters + New's clamps, as called by
 * buildSizedBloomFilter with n = max(len(set), 1) (ingest.go:139-140).  Pure host
 * arithmetic for non-Go hosts; a Go host keeps calling bloom.EstimateParameters so
 * libm differences can never change (m, k). ---- */
BSG_API int32_t bsg_estimate_parameters(uint64_t n, double false_positive_rate, uint64_t *m, uint64_t *k);

/* ---- construct ---- */

/* h[e] = bloom/v3 baseHashes(entry e): (murmur3_x64_128(d), murmur3_x64_128(d || 0x01)), seed 0.
 * entry e = bytes[offsets[e] .. offsets[e+1]).  out_h: n_entries * 4 u64. */
BSG_API int32_t bsg_hash_entries(bsg_ctx *ctx, const uint8_t *bytes, const uint32_t *offsets,
                                 uint32_t n_entries, uint64_t *out_h);

/* Build n_filters bitsets in one pass.  Entries are grouped by filter:
 * filter f owns entries [filter_entry_start[f], filter_entry_start[f+1]).
 * desc[f] gives (m, k) (computed by the caller, see above) and word_off into
 * out_words, which the callee zero-fills and then populates: for every entry
 * and i < k, bit (location(h, i) mod m) is set.  Result is a pure function of
 * (entry set, m, k) — insertion order is irrelevant, exactly as for AddString. */
BSG_API int32_t bsg_build(bsg_ctx *ctx, const uint8_t *bytes, const uint32_t *offsets, uint32_t n_entries,
                          const uint32_t *filter_entry_start, const bsg_filter_desc *desc, uint32_t n_filters,
                          uint64_t *out_words, uint64_t n_words);

/* Same, from pre-computed base hashes (n_entries * 4 u64). */
BSG_API int32_t bsg_build_hashed(bsg_ctx *ctx, const uint64_t *h, uint32_t n_entries,
                                 const uint32_t *filter_entry_start, const bsg_filter_desc *desc,
                                 uint32_t n_filters, uint64_t *out_words, uint64_t n_words);

/* ---- probe ---- */

/* Upload the filters of n_blocks blocks: desc[b*3 + kind].  Blocks are sharded
 * round-robin over the context's devices (block b -> device b % n_devices). */
BSG_API int32_t bsg_arena_load(bsg_ctx *ctx, const uint64_t *words, uint64_t n_words,
                               const bsg_filter_desc *desc, uint32_t n_blocks, uint64_t *out_arena_id);
/* Same, straight from the on-disk bytes: section b = region[sec_off[b] .. sec_off[b+1]) exactly as
 * encodeFilterSection wrote it (file_format.go:343-384; an empty range = block without filters).
 * Everything inside a section — CRC32C, flags, lengths, (m, k), the big-endian words — is parsed and decoded on the
 * device; the host never looks inside.  out_status[b]: 0 ok, else parseFilterSection's failure for that block (-1 too
 * small, -2 CRC mismatch = ErrInvalidHash, -3 unknown flags, -4 truncated, -5 bad filter, -6 trailing bytes, -7 the
 * section's bytes were never completely handed over); a failed block gets nil filters and never poisons the others
 * (query_exec.go:580-590).  Deviations from bloom/v3 ReadFrom, both "bad filter": a bitset shorter than m, and
 * k > 1024 (a corrupt section with a valid CRC must not make a probe loop 2^32 times).  Contexts on several devices
 * shard the blocks round-robin as bsg_arena_load does. */
BSG_API int32_t bsg_arena_load_sections(bsg_ctx *ctx, const uint8_t *region, uint64_t region_len, const uint64_t *sec_off,
                                        uint32_t n_blocks, int32_t *out_status, uint64_t *out_arena_id);
/* The same load as the reference's region cursor performs it (blockFilterCursor / planBlockFilterReads,
 * file_format.go:511-662): the host hands the file's filter region over in the chunks it reads (<= 4 MiB each in the
 * reference), in any order, skipping what it does not need; a section is decoded as soon as its last byte has
 * arrived, while the next chunk is still being copied.
 *   begin : sec_begin[b] / sec_end[b] = FILE offsets of candidate block b's section (equal = no section)
 *   append: bytes[0 .. len) = file bytes [file_offset, file_offset + len); copied out before the call returns.  Ranges that
 *           were handed over before are ignored: a byte's FIRST delivery is final (a re-read after a bad read must go
 *           through a new stream)
 *   finish: out_status[n_blocks] as above, the arena id; the stream id is consumed (abort discards it instead) */
BSG_API int32_t bsg_arena_stream_begin(bsg_ctx *ctx, const uint64_t *sec_begin, const uint64_t *sec_end, uint32_t n_blocks,
                                       uint64_t *out_stream_id);
BSG_API int32_t bsg_arena_stream_append(bsg_ctx *ctx, uint64_t stream_id, uint64_t file_offset, const uint8_t *bytes, uint64_t len);
BSG_API int32_t bsg_arena_stream_finish(bsg_ctx *ctx, uint64_t stream_id, int32_t *out_status, uint64_t *out_arena_id);
BSG_API int32_t bsg_arena_stream_abort(bsg_ctx *ctx, uint64_t stream_id);
BSG_API int32_t bsg_arena_free(bsg_ctx *ctx, uint64_t arena_id);

/* ---- resident file arenas across queries ----
 * The reference re-reads and re-parses a file's block-filter sections on every query (blockFilterCursor, file_format.go:511-662;
 * evaluateBlockFilters, query_exec.go:546-615).  Here a file's decoded filters stay on the device between queries, under one
 * policy inside the library: least recently used by BYTES against a budget, an arena somebody holds a lease on is never evicted,
 * only clean decodes become resident, a miss widens the resident arena to the union of the block sets, a tombstoned file
 * (merge.go:178-185) is forgotten at once and freed by its last user.
 *   key            the file's identity (MaybeFile.Pointer bytes)
 *   block_keys     strictly ascending u64 per candidate block (DataBlockMetadata.RowDataOffset, the order evaluateBlockFilters
 *                  walks them in); row i of a published arena holds block_keys[i]
 *   acquire        covered: *out_lease != 0, *out_arena_id, *out_arena_blocks (may be NULL) = blocks the arena holds (its survivor
 *                  rows have ceil(that / 64) words), out_rows[i] = candidate i's row (block index) in that arena;
 *                  not covered: *out_lease == 0 — load (have + own candidates), publish
 *   have           cap == 0: *out_n only; else the resident arena's block keys and section extents (file offsets)
 *   publish        arena_id from bsg_arena_stream_finish / bsg_arena_load_sections of exactly these blocks, status = its out_status
 *                  (NULL: all clean).  The cache OWNS the arena from here on (bsg_arena_free on it is BSG_E_INVALID); the returned
 *                  lease keeps it alive for this query whether or not it became resident (*out_resident).
 *   release        ends a lease (unknown / already released: BSG_E_NOTFOUND)
 * Thread-safe; device memory is freed outside the cache's lock. */
typedef struct bsg_arena_cache_stats {
    uint64_t budget_bytes, resident_bytes, resident_files, leases;
    uint64_t leased_dead_bytes;      /* arenas alive only through leases (evicted-from-table, dirty, narrower, forgotten while in use) */
    uint64_t hits, misses, published, widenings, evictions, forgotten;
    uint64_t rejected_dirty, rejected_over_budget, rejected_narrower;
} bsg_arena_cache_stats;
BSG_API int32_t bsg_set_arena_budget(bsg_ctx *ctx, uint64_t bytes);
BSG_API int32_t bsg_file_arena_acquire(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, const uint64_t *block_keys, uint32_t n_blocks,
                                       uint64_t *out_lease, uint64_t *out_arena_id, uint32_t *out_arena_blocks, uint32_t *out_rows);
BSG_API int32_t bsg_file_arena_have(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, uint64_t *out_block_keys, uint64_t *out_sec_begin,
                                    uint64_t *out_sec_end, uint32_t cap, uint32_t *out_n);
BSG_API int32_t bsg_file_arena_publish(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len, uint64_t arena_id, const uint64_t *block_keys,
                                       const uint64_t *sec_begin, const uint64_t *sec_end, const int32_t *status, uint32_t n_blocks,
                                       uint64_t *out_lease, int32_t *out_resident);
BSG_API int32_t bsg_file_arena_release(bsg_ctx *ctx, uint64_t lease);
BSG_API int32_t bsg_file_arena_forget(bsg_ctx *ctx, const uint8_t *key, uint32_t key_len);
BSG_API int32_t bsg_arena_cache_stats_read(bsg_ctx *ctx, bsg_arena_cache_stats *out, int32_t reset);

/* Compile + upload a batch of queries: n_terms distinct terms and, per query q,
 * the postfix program prog_ops[prog_off[q] .. prog_off[q+1]).  No limit on the batch: one launch holds ~22 000 distinct terms
 * of a kind and ~100 verdict words per 256-query chunk, and a batch beyond that is cut — inside the library — into runs of
 * queries that probe one after the other (the caller sees one batch and one result; evaluateBloomExpression has no such limit,
 * query_exec.go:89-126).  Only a SINGLE query beyond those limits is BSG_E_UNSUPPORTED, and such a batch cannot leave its
 * survivors at a device pointer (bsg_probe_many_dev). */
BSG_API int32_t bsg_batch_create(bsg_ctx *ctx, const bsg_term *terms, uint32_t n_terms,
                                 const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                 uint64_t *out_batch_id);
BSG_API int32_t bsg_batch_free(bsg_ctx *ctx, uint64_t batch_id);

/* Evaluate every query of the batch against every block of the arena.
 * out_survivors[q * ceil(n_blocks/64) + (b >> 6)] bit (b & 63) == 1  <=>  block b
 * survives query q (evaluateBloomFilters returned true).  out_survivors may be
 * NULL to leave the result on the device (benchmarks). */
BSG_API int32_t bsg_probe_batch(bsg_ctx *ctx, uint64_t arena_id, uint64_t batch_id, uint32_t flags,
                                uint64_t *out_survivors);

/* Probe the same batch against each of n_arenas arenas (e.g. the candidate files of one query
 * stage) in one call.  Up to 1 024 arenas (bsg_set_probe_group; at most 4 096) are covered by ONE dispatch — a 35 MB arena streams in
 * about the time a dispatch takes to ramp up and complete, so per-arena launches cap the HBM roofline fraction near
 * one half — and dispatches are software-pipelined: the program evaluation of group i rides inside the launch that
 * streams group i+1's bitsets (k_probe_fused).  out_survivors == NULL: enqueue only (results stay on the device; pair
 * with bsg_sync).  Otherwise the call is synchronous (unless BSG_PROBE_ASYNC is set on a single-device context: then
 * out_survivors must be C memory that stays valid until the next bsg_sync) and arena i's survivors ([n_queries][ceil(n_blocks_i / 64)] u64)
 * are written back to back in arena order; they leave the device on a copy stream while the next group is being
 * probed (pass memory from bsg_pinned_alloc for a plain DMA).  Contexts opened on several devices probe their shards
 * concurrently and interleave the shards' bitsets on the host. */
BSG_API int32_t bsg_probe_many(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id,
                               uint32_t flags, uint64_t *out_survivors);
/* Same, survivors left at a DEVICE pointer (single-device contexts; one-process-per-GPU layers that forward them). */
BSG_API int32_t bsg_probe_many_dev(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id,
                                   uint32_t flags, void *d_out_survivors);
/* Arenas one probe dispatch may cover (1..4096; 0 = the default, 1 024).  Up to 128 arena records ride in the dispatch's kernel
 * arguments; a larger group uploads its records into device memory in front of the dispatch (same stream). */
BSG_API int32_t bsg_set_probe_group(bsg_ctx *ctx, uint32_t max_arenas_per_launch);

/* ---- survivor ROWS: surviving block ids for the host, not Q x B / 8 bytes whatever they hold ----
 * bsg_probe_many with the host-side gather of the north star in mind (query_exec.go:321,603: the consumer walks the surviving
 * block INDICES of a query).  Per (arena i, query q) a header out_hdr[i * n_queries + q] = tag << 30 | surviving-block count and
 * the row's slot out_rows[row offset as in bsg_probe_many] whose content depends on the tag:
 *   BSG_ROW_NONE   no block survives: slot untouched          BSG_ROW_ALL    every block survives: slot untouched
 *   BSG_ROW_LIST   count <= 2 * ceil(n_blocks / 64): the slot starts with `count` ascending block indices (u32)
 *   BSG_ROW_DENSE  the slot holds the row's words exactly as bsg_probe_many writes them
 * Both buffers are written BY THE DEVICE (k_survivor_rows) and must be page-locked C memory (bsg_pinned_alloc /
 * bsg_host_register): only the bytes written cross PCIe — a batch whose rows are mostly NONE / ALL / short lists costs 4 bytes
 * per row instead of n_blocks / 8.  Flags as bsg_probe_many (with BSG_PROBE_ASYNC both buffers must stay valid
 * until bsg_sync).  bsg_survivor_row_list expands one row to its ascending block indices whatever its tag.
 * BSG_PROBE_ROWS_PACKED (round 6): a store into host memory that does not fill a line is one PCIe write of its own, and the dense
 * layout makes one per LIST row.  With the flag the payloads of every run of 256 consecutive queries (q / 256) of an arena lie back
 * to back, in query order, from the start of the run's slot area out_rows[row offset of the run's first query]: a LIST row takes
 * ceil(count / 2) words (its ids, u32), a DENSE row ceil(n_blocks / 64) words, NONE / ALL rows nothing — a row's payload begins
 * where the payloads of the run's earlier rows end, which the run's headers tell.  The headers shrink too: ONE BYTE per row at byte
 * (i * n_queries + q) of out_hdr (device d's slice: from byte d * n_arenas * n_queries), tag << 6 | count of a LIST row (at most
 * 32); an ALL row counts the arena's blocks, a DENSE row the bits of its words.  Buffer sizes as without the flag (the packed form
 * uses the front of both); arenas of at most 1 024 blocks per device (BSG_E_UNSUPPORTED beyond, before anything is launched).
 * bsg_survivor_rows_list_packed reads such rows (and answers BSG_E_UNSUPPORTED for the same arenas: nothing packed was written for them). */
#define BSG_ROW_NONE  0u
#define BSG_ROW_ALL   1u
#define BSG_ROW_LIST  2u
#define BSG_ROW_DENSE 3u
BSG_API int32_t bsg_probe_many_rows(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, uint32_t flags,
                                    uint64_t *out_rows, uint32_t *out_hdr);
BSG_API int32_t bsg_survivor_row_list(uint32_t hdr, const uint64_t *row, uint32_t n_blocks, uint32_t *out_blocks, uint32_t cap,
                                      uint32_t *out_n);
/* On a context of nd > 1 devices — the Go host's shape: ONE process that opens all 8 GPUs — every device writes the rows of ITS shards
 * (local block numbers: local l on device d is global block l * nd + d) into a slice of its own of the same two buffers:
 *   headers: out_hdr + d * n_arenas * n_queries, [arena][query] (count = the shard's surviving blocks)
 *   rows   : device d's slice behind the slices of the devices before it; in it arena i's [n_queries][ceil(local blocks / 64)] slots
 * bsg_survivor_rows_size gives the words / headers the two buffers must hold (nd == 1: the layout described above), and
 * bsg_survivor_rows_list — the north star's "host-side gather of surviving block IDs" (query_exec.go:603) — merges the nd shards'
 * rows of one (arena, query) into the ascending GLOBAL block indices: NONE shards contribute nothing, ALL shards every block they
 * hold, neither touches the rows' payload.  (Single-row, single-device: bsg_survivor_row_list above.) */
BSG_API int32_t bsg_survivor_rows_size(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id,
                                       uint64_t *out_row_words, uint64_t *out_hdr_words);
BSG_API int32_t bsg_survivor_rows_list(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, const uint64_t *rows,
                                       const uint32_t *hdr, uint32_t arena_index, uint32_t query, uint32_t *out_blocks, uint32_t cap,
                                       uint32_t *out_n);
BSG_API int32_t bsg_survivor_rows_list_packed(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas, uint64_t batch_id, const uint64_t *rows,
                                              const uint32_t *hdr, uint32_t arena_index, uint32_t query, uint32_t *out_blocks, uint32_t cap,
                                              uint32_t *out_n);

/* One-shot convenience: batch_create + probe_batch + batch_free. */
BSG_API int32_t bsg_probe(bsg_ctx *ctx, uint64_t arena_id, const bsg_term *terms, uint32_t n_terms,
                          const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                          uint64_t *out_survivors);

/* One interactive Query() in ONE call — strings in, survivors out (Query -> evaluateBlockFilters, query_exec.go:201-225, 572-615).
 * Term t = the probed STRING term_bytes[term_off[t] .. term_off[t + 1]) (Field, Token, or Field + "::" + Token) and its filter
 * kind; programs as for bsg_batch_create; out_survivors as for bsg_probe_many (arena i's [n_queries][ceil(n_blocks_i / 64)] words
 * back to back).  The strings are hashed on the host inside the call (TestString hashes inside the call too — a device launch for
 * three strings costs more than the probe), and for <= 16 distinct terms, <= 256 queries whose lowered programs hold <= 128
 * words in all, and <= 32 arenas per device, the hashes and programs ride in the kernel arguments of ONE dispatch per device
 * (k_query_direct): no batch object, nothing uploaded, survivors written straight into page-locked memory with a doorbell.
 * Anything larger takes the batch path inside the same call.  Re-entrant like every other entry point. */
BSG_API int32_t bsg_query(bsg_ctx *ctx, const uint64_t *arena_ids, uint32_t n_arenas,
                          const uint8_t *term_bytes, const uint32_t *term_off, const uint32_t *term_kinds, uint32_t n_terms,
                          const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, uint64_t *out_survivors);

/* Concurrent bsg_query calls on one context SHARE dispatches (the reference consults every candidate file of a Query() from a worker
 * goroutine of its own, query_exec.go:303-357, 427-431, and runs several Query() calls at once — mirrored call by call that is one
 * ~8 us dispatch per (query, file), serialised on the device's stream).  A call that finds the device idle goes alone, at once, as
 * described above.  Calls that arrive while another is collecting or in flight queue inside the library; the head of the queue
 * collects everything queued as (call, arena) pairs: an arena asked enough in the cycle (8 three-term queries per 35 KB of filters per block) is STREAMED once for
 * all of them (their query sets merged into one batch, each distinct term probed once: k_probe_terms + k_eval_programs), every other
 * pair is a job of ONE k_query_jobs dispatch (gather regime: cost follows the pairs asked for — one query, one call per candidate
 * file is a list of such jobs).  The collector hands its role on (two cycles in flight) and deals every caller its rows.  Nobody
 * waits for a window to fill; results equal the solo path's bit for bit.  Calls beyond 16 terms / 128 program words / 64 queries /
 * 32 arenas always go alone (the combiner's lab switches: bloomgpu_lab.h).  bsg_query_stats_read: how calls were served. */
typedef struct bsg_query_stats {
    uint64_t calls;                /* bsg_query calls that were eligible for combining                      */
    uint64_t solo_calls;           /* ... served by a dispatch of their own                                */
    uint64_t cycles;               /* collector cycles (a solo call is a cycle of one)                      */
    uint64_t cycle_calls;          /* calls served by those cycles                                          */
    uint64_t dispatches;           /* dispatches (per device) the combined cycles enqueued: hot arenas + job lists */
    uint64_t hot_arenas;           /* ... of which arenas streamed once for all their callers               */
    uint64_t max_calls_per_cycle;
    /* the combined cycles' phases on their collectors' clocks, summed (ns): merging + planning the batches; enqueueing (tables up,
     * dispatches); waiting for the device; dealing the rows out + releasing the callers (ns_wake: the releasing part of that) */
    uint64_t ns_prepare;
    uint64_t ns_enqueue;
    uint64_t ns_wait;
    uint64_t ns_deal;
    uint64_t ns_wake;
    uint64_t ns_scatter;           /* parts of ns_deal: rows copied out ...                                */
    uint64_t ns_free;              /* ... scratch given back ...                                            */
    uint64_t ns_retire;            /* ... slot released + next collector appointed                          */
} bsg_query_stats;
BSG_API int32_t bsg_query_stats_read(bsg_ctx *ctx, bsg_query_stats *out, int32_t reset);

/* The surviving blocks of ONE query as the reference's probe hands them on: blockScanCandidate{index} per survivor in the order
 * the blocks were consulted (ascending RowDataOffset, query_exec.go:321, 603) = the ascending bit positions of the query's row
 * survivor_row[ceil(n_blocks / 64)] of a bsg_probe* / bsg_query result, for an arena loaded in that block order.  out_blocks may be
 * NULL to ask for the count.  Host arithmetic, no context. */
BSG_API int32_t bsg_survivor_list(const uint64_t *survivor_row, uint32_t n_blocks, uint32_t *out_blocks, uint32_t cap, uint32_t *out_n);

BSG_API int32_t bsg_timing_read(bsg_ctx *ctx, bsg_timing *out, int32_t reset);
/* Device time (the dispatch's own start/stop timestamps) of the most recent k_build / k_hash_entries /
 * k_decode_sections launch made through bsg_build* / bsg_hash_entries / bsg_arena_load_sections (the slowest device
 * of the call, when it was cut over several; any pointer may be NULL). */
BSG_API int32_t bsg_last_kernel_ms(bsg_ctx *ctx, float *build_ms, float *hash_ms, float *decode_ms);

/* ---- fixed-geometry OR-reduce (extension) ----
 * All present filters of `kind` in the arena must share (m, k).  out_words
 * (ceil(m/64) u64) receives their bitwise OR == build(union of entry sets, m, k). */
BSG_API int32_t bsg_or_reduce(bsg_ctx *ctx, uint64_t arena_id, uint32_t kind, uint64_t *out_words, uint64_t n_words);

/* Device-pointer helper for the one-process-per-GPU layer (torch.distributed all_gather of
 * partial bitsets, then a local OR): d_dst[i] |= d_src[s*n_words + i] for s < n_src.
 * Pointers are device pointers on the context's first device. */
BSG_API int32_t bsg_or_words_dev(bsg_ctx *ctx, void *d_dst, const void *d_src, uint64_t n_words, uint32_t n_src);
/* Per-device partial OR left on the device: writes n_words u64 at d_out. */
BSG_API int32_t bsg_or_reduce_dev(bsg_ctx *ctx, uint64_t arena_id, uint32_t kind, void *d_out, uint64_t n_words);
/* Device time of the most recent k_or_reduce_blocks dispatch (the slowest device's). */
BSG_API int32_t bsg_last_or_ms(bsg_ctx *ctx, float *or_ms);

/* ---- the OR-reduce across GPUs: RCCL over xGMI inside the library (a Go host cannot call torch.distributed) ----
 * RCCL has no bitwise-OR reduction: the all-reduce is reduce-scatter + all-gather with the OR done by a kernel of the library —
 * slice j of every rank's partial bitset travels to rank j (grouped ncclSend / ncclRecv, one slice per point-to-point link),
 * is OR-ed there, and the reduced slices are ncclAllGather-ed: 2 (world - 1) / world of the bitset per GPU on the wire.  librccl is bound
 * at run time; without it these calls fail with BSG_E_UNSUPPORTED and everything else keeps working.  (BSG_RCCL_LIBRARY in the
 * environment names the library the communicator symbols are bound from instead: an RCCL build under test, or the suite's
 * in-process loopback, tests/loopback_ccl.cpp, through which one GPU runs the world > 1 schedule.)
 *   one process per GPU : rank 0 calls bsg_comm_unique_id and hands the 128 bytes to the other ranks (any channel);
 *                         every rank calls bsg_comm_init(ctx, id, rank, world) on its single-device context.
 *   one process, N GPUs : bsg_comm_init(ctx, NULL, 0, 0) makes every device of the context a rank (ncclCommInitAll).
 * bsg_or_allreduce = bsg_or_reduce over the whole communicator: every rank's out_words receives the same bitset. */
#define BSG_COMM_ID_BYTES 128
BSG_API int32_t bsg_comm_unique_id(uint8_t *out_id);
BSG_API int32_t bsg_comm_init(bsg_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world);
BSG_API int32_t bsg_comm_destroy(bsg_ctx *ctx);
/* What the communicator library itself reports for the context's (first) communicator — ncclCommCount / ncclCommUserRank:
 * the ranks RCCL sees, not the numbers the caller passed to bsg_comm_init.  *from_library = 0 when the bound library lacks
 * the two symbols (the values of bsg_comm_init are returned then).  Any out pointer may be NULL. */
BSG_API int32_t bsg_comm_info(bsg_ctx *ctx, int32_t *out_world, int32_t *out_rank, int32_t *from_library);
BSG_API int32_t bsg_or_allreduce(bsg_ctx *ctx, uint64_t arena_id, uint32_t kind, uint64_t *out_words, uint64_t n_words);
/* In place on device memory: d_words[i] = n_words u64 on the context's device i (one pointer for a single-device context). */
BSG_API int32_t bsg_or_allreduce_dev(bsg_ctx *ctx, void *const *d_words, uint64_t n_words);

/* ---- filter sections written on the device (encodeFilterSection, file_format.go:343-384) ----
 * Section b = the three filters desc[3b .. 3b+2] (m == 0 => absent, flag bit clear):
 *   [u8 flags] { [u32 LE 24 + 8 nw] [u64 BE m] [u64 BE k] [u64 BE m] [nw x u64 BE words] }* [u32 LE CRC32C of all before]
 * byte for byte what bloom/v3 WriteTo + the reference's framing produce, so the host appends the region to the file
 * as it is.  bsg_sections_size tells how large out_region must be (a function of the geometry alone). */
BSG_API int32_t bsg_sections_size(const bsg_filter_desc *desc, uint32_t n_blocks, uint64_t *out_total);
/* bsg_build followed by the encode, without the words crossing PCIe: n_filters = 3 * n_blocks; n_words sizes the
 * device arena the descriptors' word_off address; out_sec_off[n_blocks + 1] receives each section's byte offset. */
BSG_API int32_t bsg_build_sections(bsg_ctx *ctx, const uint8_t *bytes, const uint32_t *offsets, uint32_t n_entries,
                                   const uint32_t *filter_entry_start, const bsg_filter_desc *desc, uint32_t n_filters,
                                   uint64_t n_words, uint8_t *out_region, uint64_t region_cap, uint64_t *out_sec_off);
/* Device time of the most recent k_encode_payload + k_crc_sections pair (the slowest device's). */
BSG_API int32_t bsg_last_encode_ms(bsg_ctx *ctx, float *encode_ms);

/* ---- pinned host memory ----
 * Every entry point accepts ordinary (pageable) host pointers.  A host that marshals its rows, entries or sections
 * straight into a buffer from bsg_pinned_alloc (cgo: C memory, fill it through unsafe.Slice) gets asynchronous DMA at
 * the link's full rate instead of the driver's staged copy (measured: bsg_ingest_* of 1 M rows / 254 MB end to end
 * 23 -> 11 ms). */
BSG_API int32_t bsg_pinned_alloc(bsg_ctx *ctx, uint64_t n_bytes, void **out_ptr);
BSG_API int32_t bsg_pinned_free(bsg_ctx *ctx, void *ptr);
/* Page-lock memory the caller already owns (C memory, an mmap of a file or of shared memory; never Go-heap memory). */
BSG_API int32_t bsg_host_register(bsg_ctx *ctx, void *ptr, uint64_t n_bytes);
BSG_API int32_t bsg_host_unregister(bsg_ctx *ctx, void *ptr);

/* ---- tokenizers of the separator family ----
 * tokens(text) = strings.FieldsFunc(lower ? strings.ToLower(text) : text, isSep), where isSep(r) holds for an ASCII r whose bit
 * is set in sep_ascii and, under BSG_TOK_UNICODE_SPACE, for r >= 0x80 with unicode.IsSpace(r).  The text is leafTokenInput's
 * (a string's decoded text, a number's raw literal, true / false); keys and paths are never tokenized.  Separators are tested
 * AFTER lowering (U+212A KELVIN SIGN lowers to 'k', U+0130 to 'i'; under BSG_TOK_LOWER an upper-case ASCII separator never
 * occurs).  BasicWhitespaceLowerTokenizer = strings.Fields(strings.ToLower(v)) is the member bsg_tokenizer_default returns:
 * tab, LF, VT, FF, CR and space, UNICODE_SPACE | LOWER.  A NULL spec means that default.  BSG_E_INVALID: bit 0 (NUL), a
 * non-zero `reserved`, unknown flags, an n-gram width of 1 or above 4.  Separators are ASCII only.
 *
 * N-gram tokens.  flags bits 8-10 hold a width n: 0 (the words themselves, every spec without the field) or 2, 3, 4.  For n > 0
 *   tokens(text) = concat over w in FieldsFunc(lower ? ToLower(text) : text, isSep) of grams(w, n)
 * where, with o_0 < ... < o_L = len(w) the byte offsets of w's runes as Go's `range` decodes them (an invalid byte is one rune
 * of width 1: its byte without LOWER, EF BF BD under LOWER), grams(w, n) = [w] if L <= n (a short word stays searchable as
 * itself) and w[o_i : o_(i+n)] for i = 0 .. L - n otherwise.  Windows never cross a separator; an empty separator set gives the
 * n-grams of the whole leaf text, spaces included.  A window is at most 16 bytes.  Every call that takes a bsg_tokenizer accepts
 * the width (bsg_ingest_rows_tok, bsg_ingest_open and its appends, bsg_match_rows_tok, _many, _many_regex, _wide, _wide_rows,
 * _lookup, _lookup_rows, _lookup_regex, _lookup_regex_rows).
 * Condition tokens are still compared LITERALLY with the row's tokens: the matcher does not cut a condition's token into windows.
 *
 * Substring conditions.  With fold(x) = strings.ToLower(x) under BSG_TOK_LOWER (the per-rune table the tokenizers use), else x:
 *   Substring(needle) holds for a row that has a leaf whose candidate text T (leafTokenInput: a string's decoded text, a number's
 *     raw literal, true / false; never null, never a key) satisfies bytes.Contains(fold(T), fold(needle));
 *   FieldSubstring(field, needle) is the same over the leaves whose path EQUALS the field (FieldToken's leaf rule, not
 *     FieldRegex's prefix rule: the bloom side can only prune with field::token keys, which exist for the leaf's own path).
 * The exact test ignores separators and the n-gram width.  A needle is non-empty valid UTF-8 of at most 64 bytes after folding:
 * BSG_E_INVALID (empty, invalid UTF-8) or BSG_E_UNSUPPORTED (too long) before anything is launched.
 * The tokens such a row must hold, which the probe side prunes with (bloomsearch_host.h bsh_substring_terms / bsh_prune_query_sub):
 * fold the needle, split it at the spec's separators (tested on the folded runes); a word is WHOLE when the needle has a
 * separator on both of its sides, else PARTIAL (the text may continue it).  A whole word gives itself (n = 0) or grams(word, n);
 * a partial word gives nothing for n = 0 or fewer than n runes, else all its n-rune windows.  Terms are deduplicated in
 * first-occurrence order; each condition is And(Token(t) ..) or And(FieldToken(field, t) ..) over its terms, without terms
 * Field(field) or, for Substring, the always-true nil condition.  A partial word shorter than n never becomes a term: in a row it
 * is part of a longer word, whose set holds that word's windows and not the needle.
 * The AND of the terms is a candidate test only (the windows may sit in different words); bsg_match_rows_substr and
 * bsg_match_rows_many_substr decide exactly.
 *
 * Range conditions.  FieldRange(field, lo, hi, flags) (BSG_KIND_FIELD_RANGE; entry 2i + 1 is exactly BSG_RANGE_ENTRY_BYTES bytes: any
 * other length, or a flag bit above 3, is BSG_E_INVALID naming the condition) holds for a row that has a NUMBER leaf whose path
 * EQUALS the field (FieldToken's leaf rule, not FieldRegex's "at or beneath"; an array's elements lie under the array's path and each
 * is a leaf of its own) and whose value lies inside the interval.  A bound is closed, open (BSG_RANGE_LO_OPEN / _HI_OPEN) or absent
 * (BSG_RANGE_NO_LO / _NO_HI); nothing else tells intervals apart, and lo > hi is valid and never holds.
 * The value is the exact decimal value of the raw JSON literal: there is no float64 round trip (9007199254740993 is itself, 5.000
 * equals 5, 5.0001 is greater than 5), and a literal of any length is compared exactly with the int64 bounds.  Strings never hold
 * ("5" included), nor do true, false and null; an empty field never holds; a leaf without a path (a scalar at the root, a top-level
 * key "") is no candidate.
 * A literal with an exponent part (1e3, 1E+21, 2.5e-7) is not decided on the device: on a leaf whose path equals the field of ANY
 * range condition of the table it makes the row a fallback row (bloomsearch_host.h bsh_match_row_range decides every literal
 * exactly); on any other leaf it changes nothing.
 * The probe side prunes a range condition with Field(field) — a leaf's own path is a field-existence entry of the filters — under
 * the rules of the substring guard (bsh_prune_query_range): a nil condition is dropped from an And and kept in an Or. */
#define BSG_TOK_UNICODE_SPACE 1u   /* runes >= 0x80 with unicode.IsSpace end a word too */
#define BSG_TOK_LOWER         2u   /* the text is lower-cased first (unicode.ToLower per rune, as strings.ToLower) */
#define BSG_TOK_NGRAM_SHIFT   8u   /* flags bits 8-10: the n-gram width, 0 (none), 2, 3 or 4 */
#define BSG_TOK_NGRAM_MASK    0x700u
#define BSG_TOK_NGRAM(n)      (((uint32_t)(n) << BSG_TOK_NGRAM_SHIFT) & BSG_TOK_NGRAM_MASK)
typedef struct bsg_tokenizer {
    uint64_t sep_ascii[2];  /* bit (c & 63) of sep_ascii[c >> 6]: ASCII byte c (1..127) ends a word */
    uint32_t flags;         /* BSG_TOK_* | BSG_TOK_NGRAM(n) */
    uint32_t reserved;      /* 0 */
} bsg_tokenizer;
BSG_API int32_t bsg_tokenizer_default(bsg_tokenizer *out);

/* ---- device ingest: rows -> distinct bloom entries -> exact counts -> bitsets ----
 * Replaces, on the flush / merge worker, the reference's per-row host loop
 *   bloomEntrySets.indexRow (ingest.go:55-89: pathWalker.walk row_matcher.go:51-135, leafTokenInput
 *   tokenizer.go:120-133, BasicWhitespaceLowerTokenizer tokenizer.go:141-143, addFieldToken ingest.go:95-102),
 *   unionInto (ingest.go:105-115), counts (ingest.go:117-123) and buildFilters' AddString loop (ingest.go:127-145)
 * for the DEFAULT tokenizer (the reference's own fast-path check, row_matcher.go:37-40) and, through bsg_ingest_rows_tok, for
 * every tokenizer of the separator family, with or without an n-gram width (bsg_tokenizer above); tokenizers outside that
 * family stay on the host.
 * A "set" is one partition buffer's bloomEntrySets; set s owns rows
 * [set_first_row[s], set_first_row[s+1]).  A "parent" is a file-level union (flush.go:221,253);
 * parent_of_set[s] names it or is 0xFFFFFFFF.  Tables are indexed t = set * 3 + kind with parents
 * numbered after the sets (set index n_sets + p).
 *
 * Call order:  bsg_ingest_rows -> [bsg_ingest_fallback_rows -> host walker -> bsg_ingest_add_entries]
 *              -> bsg_ingest_finish (exact distinct counts; the caller sizes (m, k) with its own
 *              EstimateParameters) -> bsg_ingest_build -> bsg_ingest_free.
 * (Rows that arrive batch by batch: bsg_ingest_open / bsg_ingest_append_rows below.)
 * The device walker finishes rows of valid UTF-8 (see ingest.hip.h for the few exceptions); every other
 * row is reported by bsg_ingest_fallback_rows and MUST be walked by the host and added back with
 * bsg_ingest_add_entries before bsg_ingest_finish, or its entries are missing. */
typedef struct bsg_ingest_stats {
    uint32_t n_rows;
    uint32_t n_fallback_rows;  /* rows left to the host walker */
    uint32_t table_grows;      /* distinct-entry tables that had to be enlarged (x4 + rehash) */
    uint32_t reserved;
    uint64_t row_bytes;
    uint64_t table_bytes;      /* HBM held by the distinct-entry tables */
    float ms_walk;             /* k_ingest_rows dispatch time (sum over re-runs after a table grew; a stream: over its appends) */
    float ms_union;            /* k_ingest_union into the parents */
    float ms_build;            /* k_build_sets (+ k_bin_* for bitsets beyond LDS): first dispatch start to last dispatch end */
    float ms_encode;           /* k_encode_payload + k_crc_sections (bsg_ingest_build_sections) */
} bsg_ingest_stats;

/* flags for bsg_ingest_rows.  BSG_INGEST_TRUSTED_JSON: every row is known to be valid JSON (it came out of
 * json.Marshal, or the caller validated it): the device skips its validation pass.  Without the flag a row the
 * device walker hands back has inserted nothing; with it, such a row may already have inserted some of its
 * entries — all of which the host walker inserts again for a valid row, so the result is the same.  (An ingest opened with
 * MinMax fields also hands back rows that HAVE inserted their entries, with or without the flag: "per-set MinMax indexes" below.) */
#define BSG_INGEST_TRUSTED_JSON 1u

/* rows: marshaled JSON, row r = rows[row_off[r] .. row_off[r+1]) without a trailing newline.
 * slots_hint: optional initial table capacities [n_sets * 3] (0 = default: 256 for fields, 4 per row for
 * tokens and field::tokens); tables grow on demand, a hint only saves the re-run. */
BSG_API int32_t bsg_ingest_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set,
                                uint32_t n_parents, const uint32_t *slots_hint, uint32_t flags, uint64_t *out_ingest_id);
/* bsg_ingest_rows under a tokenizer of the separator family (tok: NULL = the default): the same arguments, chunked upload,
 * multi-device sharding and fallback rows.  A spec equal to the default runs exactly bsg_ingest_rows' kernel.  The spec is
 * recorded on the ingest; bsg_ingest_add_entries does not use it (the caller's host walker tokenizes its fallback rows with
 * the same spec). */
BSG_API int32_t bsg_ingest_rows_tok(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                    const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set,
                                    uint32_t n_parents, const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok,
                                    uint64_t *out_ingest_id);
/* bsg_ingest_rows uploads the rows in chunks: the first of about this many bytes (default 64 MiB, 0 restores it), each
 * later one twice the one before up to four times this; the copy of chunk i+1 overlaps the walk of chunk i. */
BSG_API int32_t bsg_set_ingest_chunk(bsg_ctx *ctx, uint64_t bytes);
/* ---- streaming device ingest: open an ingest without rows, append batches as they arrive, build at flush ----
 * bsg_ingest_rows takes every row of a flush at once, grouped by set.  A caller whose rows arrive in batches over seconds
 * (IngestRows, ingest.go:444-450) opens an ingest, hands each batch to the device when it arrives — the row bytes leave the
 * device again when the call returns, only the distinct-entry tables stay — and finds the union and the build left at flush time.
 * Call order:  bsg_ingest_open -> { [bsg_ingest_add_sets] -> bsg_ingest_append_rows -> [host walker -> bsg_ingest_add_entries] }*
 *              -> bsg_ingest_finish -> bsg_ingest_build | bsg_ingest_build_sections -> bsg_ingest_free,
 * the last four exactly as after bsg_ingest_rows (resident arenas included: block i = set i).
 * A streaming ingest lives on ONE device, chosen the way a small bsg_ingest_rows call chooses one; cutting a stream over the
 * devices of a context is not supported.
 *
 * bsg_ingest_open: n_sets (may be 0) empty sets and n_parents parents; parent_of_set[n_sets] as in bsg_ingest_rows (NULL with
 * n_parents == 0).  Tables are allocated, nothing is walked.  slots_hint: optional initial capacities [n_sets * 3] (0 = default:
 * 256 slots for fields, 1 024 for tokens and field::tokens — no row count is known; tables grow on demand).  flags
 * (BSG_INGEST_TRUSTED_JSON or 0) and tok (NULL = the default tokenizer) are recorded and apply to every append. */
BSG_API int32_t bsg_ingest_open(bsg_ctx *ctx, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                                const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id);
/* n_more sets numbered after the existing ones (partitions show up while batches arrive); *out_first_new_set = the first new
 * index.  parent_of_new_set[n_more], slots_hint_new[n_more * 3] (may be NULL) as in bsg_ingest_open.  The numbering of every
 * later call (add_entries, finish, build*) stays "sets, then parents": parent p is set index n_sets + p with the n_sets of that
 * moment.  Nothing is rehashed: parents get their storage in bsg_ingest_finish. */
BSG_API int32_t bsg_ingest_add_sets(bsg_ctx *ctx, uint64_t ingest_id, uint32_t n_more, const uint32_t *parent_of_new_set,
                                    const uint32_t *slots_hint_new, uint32_t *out_first_new_set);
/* One batch: row r (rows / row_off as in bsg_ingest_rows) goes to set set_of_row[r]; the rows come in any order of sets.  The
 * upload is chunked like bsg_ingest_rows' (bsg_set_ingest_chunk).  Rows the device walker hands back are returned HERE:
 * out_fallback_rows receives their batch-local indices, ascending, *out_n_fallback their number; the caller still holds
 * exactly these rows, walks them on the host and adds their entries with bsg_ingest_add_entries before bsg_ingest_finish.
 * out_fallback_rows == NULL with fallback_cap == 0 only asks for the number.  More rows handed back than fallback_cap:
 * BSG_E_INVALID with the number in *out_n_fallback and no index written; the batch HAS been walked — every row not handed back
 * is in the tables, and (as under BSG_INGEST_TRUSTED_JSON above) the call has inserted nothing the host walker would not insert
 * again — so appending the same batch again with enough room, or walking all of it on the host, gives the same sets.
 * A call that did not deliver its list (this one, or a count-only call that found rows to hand back) leaves n_rows, row_bytes
 * and n_fallback_rows of the stats as they were — the call that delivers the list counts the batch; ms_walk and table_grows
 * count every walk.  The calls on ONE streaming ingest (add_sets, append_rows, add_entries, finish) must be serialised by the
 * caller: the set count and numbering are not guarded against a concurrent add_sets.  Different ingests may run side by side.
 * bsg_ingest_fallback_rows on a streaming ingest is BSG_E_INVALID.  bsg_ingest_stats_read sums n_rows, row_bytes,
 * n_fallback_rows, ms_walk and table_grows over the appends.
 * Before anything is launched: BSG_E_NOTFOUND unknown id; BSG_E_INVALID an ingest made by bsg_ingest_rows(_tok), an ingest
 * already finished, a set_of_row value >= the current number of sets, a parent index >= n_parents (open, add_sets), row_off
 * not monotone, null arguments.  n_rows == 0: BSG_OK, nothing is launched. */
BSG_API int32_t bsg_ingest_append_rows(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *rows, const uint64_t *row_off,
                                       uint32_t n_rows, const uint32_t *set_of_row, uint32_t *out_fallback_rows,
                                       uint32_t fallback_cap, uint32_t *out_n_fallback);
/* Row indices (ascending) the host walker must finish; rows_out may be NULL to query the count. */
BSG_API int32_t bsg_ingest_fallback_rows(bsg_ctx *ctx, uint64_t ingest_id, uint32_t *rows_out, uint32_t cap,
                                         uint32_t *n_out);
/* Entries produced by the host walker for the fallback rows: packed like bsg_hash_entries, each tagged
 * with its set (< n_sets) and kind. */
BSG_API int32_t bsg_ingest_add_entries(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *bytes, const uint32_t *offsets,
                                       uint32_t n_entries, const uint32_t *set_of_entry, const uint32_t *kind_of_entry);
/* Unions the sets into their parents and returns the exact distinct counts
 * out_counts[(n_sets + n_parents) * 3] (bloomEntrySets.counts).  out_status[n_sets + n_parents] (may be
 * NULL): 0 ok, 2 = the set cannot be represented and must be rebuilt on the host path: it met an entry whose
 * base hashes contain a zero word (probability 2^-62 per entry), a slot claim that was never completed (a wave
 * context-switched out for ~seconds between its CAS and its stores), or two DIFFERENT entries with the same four base hashes
 * (a MurmurHash3 state collision, constructible for entries of >= 24 bytes: every entry also carries a 64-bit fingerprint
 * under a per-context secret key, so the pair is noticed instead of being counted once — Go's map would count two). */
BSG_API int32_t bsg_ingest_finish(bsg_ctx *ctx, uint64_t ingest_id, uint64_t *out_counts, uint32_t *out_status);
/* desc[(n_sets + n_parents) * 3]: geometry and output offsets of every table's filter (m == 0 skips it);
 * out_words as bsg_build. */
BSG_API int32_t bsg_ingest_build(bsg_ctx *ctx, uint64_t ingest_id, const bsg_filter_desc *desc, uint64_t *out_words,
                                 uint64_t n_words);
/* As bsg_ingest_build, but the words never leave the device: every set's three filters are serialised there as one
 * filter section (see bsg_build_sections) and only the section bytes come back.  desc gives (m, k) per table (word_off
 * is ignored: the device lays the words out itself); out_sec_off[n_sets + n_parents + 1].
 * out_sets_arena_id / out_parents_arena_id (either may be NULL): the filters just built are also left RESIDENT as
 * probe arenas — "block" i of the first = set i, "block" p of the second = parent p — so the file that is being
 * written can be queried without its sections ever being uploaded or decoded again.  On a context opened on several
 * devices every device receives its blocks (b % n) device to device. */
BSG_API int32_t bsg_ingest_build_sections(bsg_ctx *ctx, uint64_t ingest_id, const bsg_filter_desc *desc, uint8_t *out_region,
                                          uint64_t region_cap, uint64_t *out_sec_off, uint64_t *out_sets_arena_id,
                                          uint64_t *out_parents_arena_id);
BSG_API int32_t bsg_ingest_stats_read(bsg_ctx *ctx, uint64_t ingest_id, bsg_ingest_stats *out);
BSG_API int32_t bsg_ingest_free(bsg_ctx *ctx, uint64_t ingest_id);

/* ---- per-set MinMax indexes computed by the device ingest (partitionBuffer.minMaxIndexes, ingest.go:444-471) ----
 * Fields: 1 to BSG_MINMAX_MAX_FIELDS distinct names of 1 to BSG_MINMAX_MAX_NAME bytes, packed like bsg_hash_entries' input
 * (field_off[n_fields + 1]).  A name is a TOP-LEVEL key of the row object compared byte for byte with the decoded key — not a
 * dotted path: {"a":{"b":1}} does not feed field "a.b", {"a.b":1} does (the reference's row[index], ingest.go:455-456).
 * One row's contribution to one field: the member's value must itself be a JSON number (a string, "5" too, true, false, null,
 * an object or an array contributes nothing); of several top-level members with the key only the LAST counts (what a Go map holds
 * after decoding); the value v is the exact decimal value of the literal (no float64 round trip) and contributes
 * min = clamp(floor(v)), max = clamp(ceil(v)), clamped to [INT64_MIN, INT64_MAX] — ConvertToMinMaxInt64 (min_max.go) for every
 * literal json.Marshal writes.  A set's index for a field is the fold of its rows' contributions (UpdateMinMaxIndex) and is
 * present only if at least one row contributed; parents get none.
 * Rows the device does not decide: the device commits a row's contributions only after it has scanned the whole row, and hands
 * the row back — contributing NOTHING — when a top-level member named by a field holds a literal with an exponent, or when any
 * top-level key contains a backslash (it could decode to a field name).  Such rows are reported through the ingest's existing
 * fallback list (bsg_ingest_fallback_rows; out_fallback_rows of bsg_ingest_append_rows), merged with the walker's own hand-backs:
 * ascending, each row once, n_fallback_rows counts the union.  The caller folds every handed-back row in on the host
 * (bsh_minmax_row, bloomsearch_host.h); folding a row the device had decided again changes nothing.
 * Amendment to BSG_INGEST_TRUSTED_JSON's note, for ingests opened with fields only: a row handed back for a MinMax reason HAS
 * inserted its bloom entries, even without the flag; it passed validation, so the host walker inserts the same entries again.
 * Rows that are not valid JSON objects: the result of their set is unspecified; no other set's result is touched.
 * With fields, the filters, counts and statuses of an ingest are bit-identical to the same call without them. */
#define BSG_MINMAX_MAX_FIELDS 8u
#define BSG_MINMAX_MAX_NAME 64u
typedef struct bsg_minmax {
    int64_t min, max;          /* 0, 0 when absent */
    uint32_t present;          /* 1: at least one row contributed */
    uint32_t reserved;
} bsg_minmax;
/* bsg_ingest_rows_tok plus the fields, which are recorded on the ingest.  Before anything is launched, BSG_E_INVALID with the
 * field named in bsg_last_error: n_fields 0 or above 8, an empty name, a name over 64 bytes, two equal names, null arrays. */
BSG_API int32_t bsg_ingest_rows_minmax(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                       const uint32_t *set_first_row, uint32_t n_sets, const uint32_t *parent_of_set,
                                       uint32_t n_parents, const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok,
                                       uint64_t *out_ingest_id, const uint8_t *field_bytes, const uint32_t *field_off,
                                       uint32_t n_fields);
/* bsg_ingest_open plus the fields: every bsg_ingest_append_rows folds its batch in; bsg_ingest_add_sets grows the result. */
BSG_API int32_t bsg_ingest_open_minmax(bsg_ctx *ctx, uint32_t n_sets, const uint32_t *parent_of_set, uint32_t n_parents,
                                       const uint32_t *slots_hint, uint32_t flags, const bsg_tokenizer *tok, uint64_t *out_ingest_id,
                                       const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields);
/* out[n_sets * n_fields], record (set, field) at set * n_fields + field; cap: the records out has room for.  Valid any time after
 * the creating call or an append, and after bsg_ingest_finish.  The parts of a call cut over several devices own disjoint sets:
 * their results are placed side by side.  BSG_E_INVALID on an ingest made without fields. */
BSG_API int32_t bsg_ingest_minmax(bsg_ctx *ctx, uint64_t ingest_id, bsg_minmax *out, uint64_t cap);
/* k_minmax_rows' dispatch time in the last bsg_ingest_rows_minmax / bsg_ingest_append_rows of an ingest with fields (summed over
 * the upload chunks; the slowest device of a call cut over several).  bsg_ingest_stats keeps its layout. */
BSG_API int32_t bsg_last_minmax_ms(bsg_ctx *ctx, float *minmax_ms);

/* ---- keyed streaming ingest: the rows of a batch partitioned ON THE DEVICE by the text of one top-level member ----
 * bsg_ingest_append_rows wants set_of_row[] from the caller, who must therefore parse every row first.  A keyed ingest is opened
 * with one partition field (a name of 1 to BSG_PARTITION_MAX_NAME bytes) and finds every row's set itself.
 * A row's partition text: the FIRST top-level member whose key equals the name byte for byte counts (later members with that key
 * are ignored; unlike the MinMax fields, where the last wins).  A string value gives the bytes between its quotes, a number its raw
 * literal exactly as written (1.0, -0 and 1e5 stay what they are: no arithmetic), true and false their four or five bytes; null, an
 * object, an array or no such member give the empty text.  Equal text is the same partition whatever the JSON type: "5" and 5
 * share a set, "" and an absent member share a set.
 * Rows the device does not decide (handed back): the member's value is a string that holds a backslash; the text is longer than
 * BSG_PARTITION_MAX_KEY bytes; a top-level key that holds a backslash stands before the member, or anywhere in a row without the
 * member (it could decode to the name).  Every other row is decided.  bsh_partition_key (bloomsearch_host.h) decides every row.
 * Rows are promised to be valid JSON objects; for another row the result of that row is unspecified (nothing outside the row's
 * words is read, and no other row's result is touched).
 * Sets: every set of a keyed ingest has a text.  Sets are numbered by first appearance — the lowest row index — among the rows the
 * device decided, across the upload chunks of a call and across calls; a text registered from the host (bsg_ingest_add_sets_keyed)
 * has its number from that moment.  An ingest holds at most BSG_PARTITION_MAX_SETS sets.  A call may meet any number of new texts:
 * the device collects them BSG_PARTITION_PENDING_SLOTS at a time, the caller sees no limit.
 * Call order: as the streaming ingest's, with bsg_ingest_append_rows_keyed / bsg_ingest_add_sets_keyed in place of
 * bsg_ingest_append_rows / bsg_ingest_add_sets (plain bsg_ingest_add_sets on a keyed ingest is BSG_E_INVALID: a set without a text
 * would break the dictionary; plain bsg_ingest_append_rows keeps working with explicit sets).  finish, build, build_sections, minmax,
 * stats_read and free are unchanged, and for the same rows in the same sets the filters, counts, statuses and MinMax records are
 * bit-identical to an ingest fed through bsg_ingest_append_rows. */
#define BSG_PARTITION_MAX_NAME 64u
#define BSG_PARTITION_MAX_KEY 128u
#define BSG_PARTITION_PENDING_SLOTS 256u
#define BSG_PARTITION_MAX_SETS (1u << 20)
#define BSG_SET_UNDECIDED 0xFFFFFFFFu
/* bsg_ingest_open with no initial sets, plus the partition field (name_bytes[name_len]), the parent every set the ingest creates
 * will have (< n_parents, or 0xFFFFFFFF for none) and, optionally, the MinMax fields of bsg_ingest_open_minmax (n_fields == 0 with
 * NULL arrays: none).  Before anything is allocated, BSG_E_INVALID with the cause in bsg_last_error: an empty name, a name over
 * BSG_PARTITION_MAX_NAME bytes, parent_of_new_sets >= n_parents, and what bsg_ingest_open(_minmax) refuses. */
BSG_API int32_t bsg_ingest_open_keyed(bsg_ctx *ctx, uint32_t n_parents, uint32_t parent_of_new_sets, uint32_t flags,
                                      const bsg_tokenizer *tok, uint64_t *out_ingest_id, const uint8_t *name_bytes, uint32_t name_len,
                                      const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields);
/* bsg_ingest_append_rows without set_of_row.  out_set_of_row[n_rows]: every row's set, or BSG_SET_UNDECIDED for a row the
 * partitioner handed back; *out_n_new_sets: the sets this call created (the ingest's last ones).  The fallback list is the ascending
 * union, each row once, of the partitioner's hand-backs, the walker's and the MinMax scanner's; the caller tells the first kind by
 * BSG_SET_UNDECIDED.  A row handed back by the partitioner has not been walked and has inserted nothing; for it the caller finds
 * the text on the host (bsh_partition_key), registers it if new (bsg_ingest_add_sets_keyed), walks the row with the host walker
 * (bsg_ingest_add_entries) and folds its MinMax values on the host — what it does for every fallback row already.
 * fallback_cap, count-only calls, the statistics, n_rows == 0 and the serialisation of calls on one ingest: as bsg_ingest_append_rows.
 * Sets created by a call whose list did not fit stay created, and out_set_of_row has been written: appending the batch again
 * gives the same sets.  The number of new texts is known before any set is created: a call that cannot give them their sets
 * (BSG_PARTITION_MAX_SETS, an allocation failure) fails and leaves the ingest as it was. */
BSG_API int32_t bsg_ingest_append_rows_keyed(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *rows, const uint64_t *row_off,
                                             uint32_t n_rows, uint32_t *out_set_of_row, uint32_t *out_n_new_sets,
                                             uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback);
/* Texts found on the host (n_keys of them, packed like bsg_hash_entries' input, key_off[n_keys + 1]; any length, any bytes):
 * out_set_of_key[i] = the set of text i — the one it has, or the next new one (equal texts within the call share it).  Later
 * batches resolve these texts to the same sets on the device. */
BSG_API int32_t bsg_ingest_add_sets_keyed(bsg_ctx *ctx, uint64_t ingest_id, const uint8_t *key_bytes, const uint32_t *key_off,
                                          uint32_t n_keys, uint32_t *out_set_of_key);
/* The texts of sets [first, n_sets), packed like bsg_hash_entries' input: out_off[*out_n_keys + 1].  *out_n_keys and *out_n_bytes
 * are always written; out_bytes == NULL with out_off == NULL asks for them alone.  Valid until bsg_ingest_free. */
BSG_API int32_t bsg_ingest_keys(bsg_ctx *ctx, uint64_t ingest_id, uint32_t first, uint8_t *out_bytes, uint64_t bytes_cap,
                                uint32_t *out_off, uint32_t *out_n_keys, uint64_t *out_n_bytes);
/* The partition kernels' (k_partition_rows, k_partition_assign) dispatch time in the last bsg_ingest_append_rows_keyed, summed over
 * its upload chunks and rounds.  bsg_ingest_stats keeps its layout. */
BSG_API int32_t bsg_last_partition_ms(bsg_ctx *ctx, float *partition_ms);

/* ---- final row test on the device (compileRowMatcher / matchRowBytes, row_matcher.go:257-626) ----
 * One expression over Field / Token / FieldToken conditions, evaluated for every row of the surviving blocks.
 * Condition i: cond_kinds[i] (BSG_KIND_*) and two strings packed like bsg_hash_entries' input — entry 2i = the FIELD
 * string (Field, FieldToken; empty for Token), entry 2i + 1 = the TOKEN string (Token, FieldToken; empty for Field):
 * cond_off[2 * n_conds + 1].  FieldToken is the (path, token) PAIR at one leaf, not the joined "path::token" key
 * (row_matcher.go:587).  prog_ops: the public postfix program over condition indices (BSG_OP_TERM i / AND n / OR n / TRUE /
 * FALSE; n_ops == 0 = nil expression = every row matches; a nil condition lowers to TRUE, an unknown condition or expression
 * type to FALSE, as evalMatcherNode does).
 * out_bits[ceil(n_rows / 64)]: bit r & 63 of word r >> 6 set <=> row r matches.  Rows the device cannot decide are listed
 * in out_fallback_rows (ascending; their bit is 0) and must be decided by the host matcher: rows outside the device
 * walker's envelope (see bsg_ingest_rows), and rows in which an emission has the base hashes of a condition string but
 * not its keyed fingerprint — a MurmurHash3 state collision, where only matchRowBytes' byte compare is exact.
 * Target tokens are never normalised (Token("ALICE") misses, row_matcher_test.go:99-100).
 * The rows of a large call are uploaded in chunks (bsg_set_ingest_chunk) on a copy stream while the chunk before is matched.
 * Limits: 64 conditions, expression depth 64 (BSG_E_UNSUPPORTED beyond). */
BSG_API int32_t bsg_match_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                               const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                               const uint32_t *prog_ops, uint32_t n_ops,
                               uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                               uint32_t *out_n_fallback);
/* The same call (same arguments, sharding, chunked upload and fallback rows) with FieldRegex conditions as well:
 * cond_kinds[i] == BSG_KIND_FIELD_REGEX, entry 2i = the field, entry 2i + 1 = the pattern, so one program holds a whole
 * compileRowMatcher root And(bloom root, regex root) (row_matcher.go:353-368).  A regex condition holds when its pattern
 * matches (Go regexp MatchString) the candidate text of any leaf whose path equals the field or starts with field + ".":
 * a string's decoded text, a number's raw literal, true / false — never null; an empty field never holds.
 * Patterns are compiled per call to byte DFAs for a stated subset of RE2 syntax (bloomsearch_amd/csrc/host/regex_dfa.hpp:
 * literals, escapes, ., classes, Perl / ASCII POSIX classes, ^ $ \A \z, groups, alternation, counted and lazy
 * repetition, flags i s U with (?i) over ASCII only); bsh_regex_match (bloomsearch_host.h) runs the same tables on the host.
 * BSG_E_UNSUPPORTED before anything is launched (message in bsg_last_error naming the construct): a pattern outside the
 * subset or whose DFA exceeds 1 024 states, more than 16 regex conditions, or tables over 44 544 bytes of LDS.  Callers
 * validate patterns with their own engine first; the device never decides that a pattern is invalid.  Rows whose leaf
 * falls under more than 4 regex conditions are fallback rows too. */
BSG_API int32_t bsg_match_rows_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                     const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                     const uint32_t *prog_ops, uint32_t n_ops,
                                     uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                     uint32_t *out_n_fallback);
/* bsg_match_rows / bsg_match_rows_regex for an engine whose tokenizer is of the separator family (tok: NULL = the default):
 * Token and FieldToken conditions compare the words of that tokenizer; FieldRegex conditions (allowed here) read the leaf
 * text and ignore it.  The condition kinds choose the kernel, a spec equal to the default runs the default kernels.  Same
 * arguments, limits, sharding, chunked upload and fallback rows as bsg_match_rows_regex. */
BSG_API int32_t bsg_match_rows_tok(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                   const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                   const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                   uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                   uint32_t *out_n_fallback);
/* bsg_match_rows_tok with substring conditions in the table (kinds 0, 1, 2, BSG_KIND_SUBSTRING, BSG_KIND_FIELD_SUBSTRING; the
 * semantics under "Substring conditions" above).  The caller passes the RAW needle as entry 2i + 1; the call folds it under its own
 * tokenizer.  The walker's text consumer runs shift-and over all needles at once: one LDS read per text byte whatever their number.
 * Same arguments, sharding, chunked upload, fallback rows and bsg_last_match_ms as bsg_match_rows_tok; a row with a rune the
 * lower table cannot decide is a fallback row (bloomsearch_host.h bsh_match_row_substring decides those), as is a row where a
 * leaf's path has the hashes of a FieldSubstring condition's field but not its fingerprint.
 * Limits: a needle of at most 64 bytes after folding; the needles are packed first-fit, in condition order, into 2 words of 64
 * bytes and a needle never straddles a word, so at most 128 needle bytes per call (BSG_E_UNSUPPORTED beyond).
 * A BSG_KIND_FIELD_REGEX condition is BSG_E_UNSUPPORTED here: regex and substring conditions share bsg_match_rows_regex_substr.
 * Every entry point but these two pairs and bsg_match_rows_wide_substr(_rows) answers kinds 4 and 5 with BSG_E_INVALID (unknown kind). */
BSG_API int32_t bsg_match_rows_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                      const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                      const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                      uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                      uint32_t *out_n_fallback);
/* bsg_match_rows_tok with range conditions in the table (kinds 0, 1, 2 and BSG_KIND_FIELD_RANGE; the semantics under "Range
 * conditions" above).  The walker's fourth text consumer parses each number leaf a range condition listens on once, whatever the
 * number of conditions on it, and compares in integer arithmetic; the bounds travel in the conditions' own records (no LDS is added:
 * k_match_rows_range* keep k_match_rows*'s bytes and workgroups per CU).  A table without a range condition runs bsg_match_rows_tok's
 * kernels and returns its bits.  Same arguments, limits, sharding, chunked upload, fallback rows and bsg_last_match_ms as
 * bsg_match_rows_tok; a row with an exponent literal on a range condition's leaf is a fallback row too, as is one where a leaf's
 * path has the hashes of a range condition's field but not its fingerprint.
 * A condition of kind 3, 4 or 5 is BSG_E_UNSUPPORTED here (the condition named): range conditions share a table with the regex and
 * substring consumers in bsg_match_rows_regex_substr_range / bsg_match_rows_many_regex_substr_range only.  Every entry point but those
 * two, this one, bsg_match_rows_many_range and bsg_match_rows_wide_range(_rows) answers kind 6 with BSG_E_INVALID (unknown kind). */
BSG_API int32_t bsg_match_rows_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                     const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                     const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                     uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                     uint32_t *out_n_fallback);
/* A batch of queries matched in ONE upload and ONE walk of the rows (k_match_rows_many): n_queries <= 64 expressions over ONE
 * table of distinct Field / Token / FieldToken conditions (packed as for bsg_match_rows), prog_ops / prog_off[n_queries + 1]
 * the public postfix programs over condition indices laid out as for bsg_batch_create (an empty program = nil expression =
 * every row matches).  out_bits holds n_queries bit-planes of ceil(n_rows / 64) words: plane q = what bsg_match_rows(_tok)
 * returns for expression q alone.
 * Rows may come grouped in sets (one surviving block each): set s = rows [set_first_row[s], set_first_row[s + 1]),
 * set_first_row[0] == 0, set_first_row[n_sets] == n_rows, and bit q of query_mask_of_set[s] says that query q survived the probe on
 * that block and is evaluated there; every other plane bit of the set's rows is 0.  NULL, NULL, 0 = every query on every row.
 * A row whose set has mask 0 is never walked.  tok: NULL = the default tokenizer, as bsg_match_rows_tok.
 * Fallback rows (listed once, ascending; all their plane bits are 0): a row with a non-zero mask that leaves the device walker's
 * envelope, or in which an emission has the base hashes of ANY table condition but not its fingerprint.  A row with mask 0 is
 * never a fallback row.  The host matcher decides them per query whose mask bit is set.
 * Limits (BSG_E_UNSUPPORTED before anything is launched): 64 queries, 64 conditions, 2 048 lowered ops over all programs
 * (an n-ary AND / OR lowers to n - 1 binary ops), depth 64 per program, and no BSG_KIND_FIELD_REGEX condition: the regex kernels
 * are sized differently (bsg_match_rows_regex).  BSG_E_INVALID: null arguments, offsets that are not monotone, a set table that
 * does not span [0, n_rows), mask bits at or above n_queries.  n_queries == 0 or n_rows == 0: BSG_OK, nothing written.
 * Sharding over the context's devices, chunked upload and bsg_last_match_ms as bsg_match_rows. */
BSG_API int32_t bsg_match_rows_many(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                    const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                    const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                    const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                    const bsg_tokenizer *tok,
                                    uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                    uint32_t *out_n_fallback);
/* bsg_match_rows_many with substring conditions in the table, as bsg_match_rows_substr documents them: the same nineteen arguments,
 * set / mask semantics, plane layout and limits as bsg_match_rows_many, the needle limits of bsg_match_rows_substr over the table's
 * DISTINCT conditions; plane q = what bsg_match_rows_substr returns for program q alone, ANDed with the set mask. */
BSG_API int32_t bsg_match_rows_many_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                           const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                           const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                           const bsg_tokenizer *tok,
                                           uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                           uint32_t *out_n_fallback);
/* bsg_match_rows_many with range conditions in the table, as bsg_match_rows_range documents them: the same nineteen arguments, set /
 * mask semantics, plane layout and limits as bsg_match_rows_many; plane q = what bsg_match_rows_range returns for program q alone,
 * ANDed with the set mask.  An exponent literal on the leaf of ANY range condition of the table makes a walked row a fallback row,
 * whatever the mask bits of the queries that use the condition; a row with mask 0 is never walked and never a fallback row. */
BSG_API int32_t bsg_match_rows_many_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                          const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                          const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                          const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                          const bsg_tokenizer *tok,
                                          uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                          uint32_t *out_n_fallback);
/* FieldRegex AND substring conditions in one table, decided in ONE walk of the rows (kinds 0-5; k_match_rows_regex_substr*): the
 * arguments of bsg_match_rows_substr, a FieldRegex condition as bsg_match_rows_regex documents it, a substring condition as
 * bsg_match_rows_substr does.  Every candidate text goes to both consumers: the DFAs read the raw bytes, the needles the folded ones.
 * A table without a FieldRegex condition is bsg_match_rows_substr's, one without a substring condition bsg_match_rows_tok's: the
 * same kernels, limits and bits.  With both kinds in the table:
 * Limits (BSG_E_UNSUPPORTED before anything is launched, the condition named): 64 conditions, 16 regex conditions with patterns in
 * the compiler's subset, regex tables of at most 40 448 bytes (what the needle table leaves of bsg_match_rows_regex's 44 544), the
 * needle limits of bsg_match_rows_substr, the program limits of bsg_match_rows.
 * Fallback rows: the union of the two parents' — the walker's envelope, a fingerprint collision, more than 4 regex conditions on
 * one leaf, a rune the lower table cannot decide.  bsh_match_row_with, bsh_match_row_regex and bsh_match_row_substring decide them. */
BSG_API int32_t bsg_match_rows_regex_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                            const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                            uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                            uint32_t *out_n_fallback);
/* The batched call of the same (k_match_rows_many_regex_substr*): the nineteen arguments, set / mask semantics and plane layout of
 * bsg_match_rows_many, the regex rules of bsg_match_rows_many_regex (a leaf opens a condition's DFA only on a row whose set mask
 * selects a query that uses it, so "more than 4 regex conditions on one leaf" counts those alone), the needle limits of
 * bsg_match_rows_substr, and regex tables (user masks included) of at most 34 032 bytes beside a needle table.  Plane q = what
 * bsg_match_rows_regex_substr returns for program q alone, ANDed with the set mask. */
BSG_API int32_t bsg_match_rows_many_regex_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                 const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                 const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                 const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                                 const bsg_tokenizer *tok,
                                                 uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                 uint32_t *out_n_fallback);
/* Range, FieldRegex and substring conditions in one table, decided in ONE walk of the rows (kinds 0-6; k_match_rows_regex_substr_range*):
 * the fifteen arguments of bsg_match_rows_regex_substr.  Every kind keeps its documented entry format and refusals: the 17-byte range
 * entry and its flag bits ("Range conditions"), the needle rules of bsg_match_rows_substr, regex conditions as bsg_match_rows_regex
 * documents them.  A number literal is candidate text of all three consumers on the same bytes: the DFAs read it raw, the needles
 * folded, the number parser as digits; a string reaches the first two alone (a string never holds for a range condition).
 * The table decides the path: without a range condition the call is bsg_match_rows_regex_substr (same kernels, caps and bits); with
 * range conditions and no condition of kind 3, 4 or 5 it is bsg_match_rows_range; any other table runs the three-consumer walkers,
 * whether its text side is needles only, regex only or both.
 * Limits of such a table (BSG_E_UNSUPPORTED before anything is launched, the condition named): 64 conditions, 16 regex conditions with
 * patterns in the compiler's subset, regex tables of at most 40 448 bytes WHETHER OR NOT the table holds a needle (the walkers always
 * carry the 4 096-byte needle table), the needle limits of bsg_match_rows_substr, the program limits of bsg_match_rows.
 * BSG_E_INVALID: a kind above 6, a range entry of another length or with flag bits above 3, an empty or invalid needle.
 * Fallback rows: the union of the parents' — the walker's envelope, a fingerprint collision, more than 4 regex conditions on one
 * leaf, a rune the lower table cannot decide, an exponent literal on a range condition's leaf.  bsh_match_row_with,
 * bsh_match_row_regex, bsh_match_row_substring and bsh_match_row_range decide them together.
 * Sharding, chunked upload, fallback list and bsg_last_match_ms as bsg_match_rows. */
BSG_API int32_t bsg_match_rows_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                  const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                  const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                                  uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                  uint32_t *out_n_fallback);
/* The batched call of the same (k_match_rows_many_regex_substr_range*): the nineteen arguments, set / mask semantics, plane layout and
 * limits of bsg_match_rows_many, and the delegation of the single call (no range condition: bsg_match_rows_many_regex_substr; range
 * conditions and no kind 3-5: bsg_match_rows_many_range).  Each family keeps its batched parent's gating: a leaf opens a regex
 * condition's DFA only on a row whose set mask selects a query that uses it, needles are not gated, and an exponent literal on the
 * leaf of ANY range condition of the table makes a walked row a fallback row whatever its mask.  Regex tables (user masks included):
 * at most 34 032 bytes, whether or not the table holds a needle.  Plane q = what bsg_match_rows_regex_substr_range returns for
 * program q alone, ANDed with the set mask. */
BSG_API int32_t bsg_match_rows_many_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                       const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                       const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                       const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                                       const bsg_tokenizer *tok,
                                                       uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                       uint32_t *out_n_fallback);
/* bsg_match_rows_many with FieldRegex conditions in the table (k_match_rows_many_regex): the same nineteen arguments, set / mask
 * semantics, plane layout, sharding over the context's devices, chunked upload and bsg_last_match_ms.  What differs:
 * - cond_kinds[i] may be BSG_KIND_FIELD_REGEX (entry 2i = the field, 2i + 1 = the pattern) with the meaning bsg_match_rows_regex
 *   documents: the pattern matches the candidate text of any leaf at or under the field, never null, an empty field never holds;
 *   under a tokenizer spec the regex still reads the leaf text, not its words.  Plane q = what bsg_match_rows_tok returns for
 *   program q alone over the same table.
 * - A table without any regex condition runs exactly bsg_match_rows_many's kernels and returns exactly its result.
 * - Limits (BSG_E_UNSUPPORTED before anything is launched, the message names the condition index and the construct): those of
 *   bsg_match_rows_many; more than 16 distinct regex conditions; a pattern outside the compiler's subset or over 1 024 states; DFA
 *   tables over 38 140 bytes of LDS (80 KiB minus the batched matcher's 43 780: 6 404 bytes less than bsg_match_rows_regex takes),
 *   of which every regex condition spends 16 header bytes, 8 bytes for the mask of the queries that use it, its class map and
 *   transitions (256 + 2 * states * classes, padded to 4) and its field string.
 * - Fallback rows: those of bsg_match_rows_many, and a row in which one leaf would feed more than 4 regex conditions at once,
 *   counting only conditions referenced by a query whose mask bit is set on the row's set (a regex condition is opened on a leaf
 *   only for rows that evaluate a query using it).  Listed once, ascending, all plane bits 0. */
BSG_API int32_t bsg_match_rows_many_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                          const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                          const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                          const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets,
                                          const bsg_tokenizer *tok,
                                          uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                          uint32_t *out_n_fallback);
/* ANY number of queries over one condition table in ONE upload and ONE walk of the rows.  The work is split as the probe side
 * splits it: the walk (k_match_rows_store*) writes every row's 64-bit condition word to device memory, k_eval_row_programs
 * evaluates the programs over those words.  The condition table (FieldRegex conditions allowed), prog_ops / prog_off[n_queries + 1]
 * and tok are exactly bsg_match_rows_many_regex's; an empty program is the nil expression: every row matches.
 * Sets: set s = rows [set_first_row[s], set_first_row[s + 1]), set_first_row[0] == 0, set_first_row[n_sets] == n_rows.  The u64 mask
 * of the batched call becomes a CSR list: set_queries[set_query_off[s] .. set_query_off[s + 1]) are the queries evaluated on set s,
 * strictly ascending, each < n_queries; set_query_off[0] == 0.  A PAIR p is an index into set_queries.  NULL, NULL, NULL, 0 = one
 * implicit set of all rows with every query: the result then has the plane layout of bsg_match_rows_many.
 * out_bits (bsg_match_wide_size says how many words): pair p of set s owns ceil(rows of s / 64) consecutive words from
 * pair_word_off[p] on, pairs in order; bit i & 63 of word i >> 6 is set <=> row set_first_row[s] + i matches the program of
 * set_queries[p] (= what bsg_match_rows_tok returns for that program alone over the same table); bits past the set's last row are
 * 0.  The result is sparse: nothing is stored for a (set, query) the caller did not list.
 * Fallback rows (listed once, ascending, all their pair bits 0), only among rows of a set with at least one pair: a row that leaves
 * the device walker's envelope; a row in which an emission has the base hashes of ANY table condition but not its fingerprint; a
 * row in which one leaf would feed more than 4 regex conditions at once, counting only conditions referenced by the program of a
 * query in the set's list.  Rows of a set with no pair are never walked and never fallback rows.
 * Limits (BSG_E_UNSUPPORTED before anything is launched): 64 distinct conditions; 16 regex conditions; the regex subset and 1 024
 * states of bsg_match_rows_regex; program depth 64; DFA tables over 46 592 bytes of LDS (80 KiB minus the storing walker's 35 328:
 * it keeps no program in LDS; per regex condition 16 header bytes, its class map and transitions (256 + 2 * states * classes,
 * padded to 4) and its field string); 1 048 576 (2^20) queries; 4 194 304 (2^22) lowered ops over all programs (an n-ary AND / OR
 * lowers to n - 1 binary ops); 16 777 216 (2^24) pairs; 2^30 (64-row tile, 64-pair range) items on one device.  Beyond that only
 * device memory bounds a call (BSG_E_NOMEM): 9 bytes per row, 4 per lowered op, query and pair, 8 per result word.
 * BSG_E_INVALID: null arguments, offsets that are not monotone, a set table that does not span [0, n_rows), a query list that is not
 * strictly ascending or names a query >= n_queries.  n_rows == 0 or zero pairs: BSG_OK, nothing written.
 * Sharding over the context's devices (parts are cut at set-relative multiples of 64 rows: no two devices write one word), chunked
 * upload and bsg_last_match_ms (the walk plus the evaluation of the slowest device) as bsg_match_rows_many. */
BSG_API int32_t bsg_match_rows_wide(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                    const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                    const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                    const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                    uint32_t n_sets, const bsg_tokenizer *tok,
                                    uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                    uint32_t *out_n_fallback);
/* The layout of bsg_match_rows_wide's result, host arithmetic without a context: out_pair_word_off[n_pairs + 1] (may be NULL) and
 * the total number of words.  NULL, NULL, 0 = the implicit set (n_pairs = n_queries).  BSG_E_INVALID as the call itself. */
BSG_API int32_t bsg_match_wide_size(const uint32_t *set_first_row, const uint32_t *set_query_off, uint32_t n_sets, uint32_t n_rows,
                                    uint32_t n_queries, uint64_t *out_pair_word_off, uint64_t *out_total_words);
/* bsg_match_rows_wide with each pair's matches delivered as a tagged row list: what the host goes on with is the rows to
 * materialise (matchRowBytes is followed at once by materializeRow, query_exec.go:751-755), not a bitmap to search, and a
 * search's answer is a handful of rows per query while the bit rows cost rows / 8 bytes per pair whatever they hold.  Every argument
 * up to and including tok, the limits, validation, sharding, chunked upload and the fallback-row rules are bsg_match_rows_wide's.
 * Pair p of set s (R rows, T = ceil(R / 64)), c of whose rows match (a fallback row never counts), gets the header
 * out_pair_hdr[p] = tag << 30 | n and, from out_payload[out_pair_off[p]] on (offsets in u32):
 *   BSG_ROW_NONE   c == 0 (every pair of a set with R == 0)   n = 0, no payload
 *   BSG_ROW_ALL    c == R, R > 0                              n = 0, no payload
 *   BSG_ROW_LIST   0 < c < R and c < 2 * T                    n = c, c ascending set-relative row indices i: row set_first_row[s] + i
 *   BSG_ROW_DENSE  otherwise                                  n = 0, 2 * T u32: word t of the pair's bit row is
 *                                                             payload[2 * t] | (uint64_t)payload[2 * t + 1] << 32, exactly the
 *                                                             words bsg_match_rows_wide returns (no alignment is promised)
 * The tag is a function of (c, R) alone and the result is the same for any number of devices and any chunk size: a set cut
 * between devices is stitched on the host into the canonical form.  Payloads lie back to back in pair order; out_pair_off
 * [n_pairs + 1] may be NULL (the host computes it from the headers: a LIST takes n, a DENSE pair 2 * T, the others nothing).  No
 * result is longer than the bit rows: payload_cap = 2 * bsg_match_wide_size's total words can never be too small.
 * *out_payload_len = the payload's u32.  payload_cap too small: every header, out_pair_off and *out_payload_len (the length
 * needed) are written, no payload is, and the call returns BSG_E_INVALID (the message names both numbers).  n_rows == 0 or zero
 * pairs: BSG_OK, every header NONE, *out_payload_len = 0.  out_payload may be NULL when payload_cap is 0.
 * On the device three passes follow the evaluation (k_pair_sizes, the k_pair_scan_* offset scan over BSG_MATCH_PAIR_SCAN_WIDTH
 * pairs per workgroup, k_pair_write); only the headers (4 bytes per pair) and the payload cross PCIe.  Device memory beyond
 * bsg_match_rows_wide's: the payload scratch is sized at its bound, 8 more bytes per result word, and 20 bytes per pair.
 * bsg_last_match_ms: the walk, the evaluation and the list passes. */
#define BSG_MATCH_PAIR_SCAN_WIDTH 256u
BSG_API int32_t bsg_match_rows_wide_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                         const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                         const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                         const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                         uint32_t n_sets, const bsg_tokenizer *tok,
                                         uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                         uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                         uint32_t *out_n_fallback);
/* bsg_match_rows_wide / bsg_match_rows_wide_rows with substring conditions allowed in the table (kinds 0-5; the storing walkers
 * k_match_rows_store_substr* / k_match_rows_store_regex_substr*): the parameter lists, sets, pairs and the implicit set, result layouts,
 * bsg_match_wide_size, bsg_match_pair_rows_list, sharding, chunked upload and bsg_last_match_ms of the two wide calls; a substring
 * condition as bsg_match_rows_substr documents it (the RAW needle as entry 2i + 1, folded under the call's tokenizer), a FieldRegex
 * condition as bsg_match_rows_wide does.  Pair p's bits = what bsg_match_rows_regex_substr returns for the program of set_queries[p]
 * alone over the set's rows.  A table without a substring condition is bsg_match_rows_wide(_rows)'s: the same kernels, limits and bits.
 * Regex conditions stay gated by the set's queries; needles are not: every needle of the table listens on every walked row.  Rows of
 * a set with no pair are never walked.
 * Limits (BSG_E_UNSUPPORTED before anything is launched, the condition named): 64 distinct conditions; 16 distinct regex conditions
 * with patterns in the compiler's subset; program depth 64; the query, op, pair and item limits of bsg_match_rows_wide; a needle of at
 * most 64 bytes after folding, the needles packed first-fit in condition order into 2 words of 64 bytes (128 needle bytes at most); regex
 * tables of at most 42 496 bytes of LDS when the table holds a needle (81 920 minus the storing walker's 35 328 and the needle table's
 * 4 096: 39 424 bytes without regex tables), 46 592 when it holds none.  BSG_E_INVALID: what bsg_match_rows_wide refuses, an empty
 * needle or one that is not valid UTF-8, a kind above 5.
 * Fallback rows, only among rows of a set with at least one pair (all their pair bits 0, never counted in a list): the union of the
 * parents' rules — the walker's envelope, a fingerprint collision with ANY table condition (a FieldSubstring condition's field
 * included), more than 4 regex conditions of the set's queries on one leaf, a rune the lower table cannot decide. */
BSG_API int32_t bsg_match_rows_wide_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                           const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                           const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                           uint32_t n_sets, const bsg_tokenizer *tok,
                                           uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                           uint32_t *out_n_fallback);
BSG_API int32_t bsg_match_rows_wide_substr_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                                uint32_t n_sets, const bsg_tokenizer *tok,
                                                uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                                uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                uint32_t *out_n_fallback);
/* bsg_match_rows_wide / bsg_match_rows_wide_rows with range conditions allowed in the table (kinds 0, 1, 2 and BSG_KIND_FIELD_RANGE; the
 * storing walkers k_match_rows_store_range*): the parameter lists, sets, pairs and the implicit set, result layouts,
 * bsg_match_wide_size, bsg_match_pair_rows_list, sharding, chunked upload and bsg_last_match_ms of the two wide calls; a range
 * condition as "Range conditions" and bsg_match_rows_range document it.  Pair p's bits = what bsg_match_rows_range returns for the
 * program of set_queries[p] alone over the set's rows.  A table without a range condition is bsg_match_rows_wide(_rows)'s: the same
 * kernels, limits and bits.  No LDS is added: the walkers keep k_match_rows_store*'s bytes and workgroups per CU, and one parse of a
 * number leaf serves every range condition on it.
 * A range condition listens on a leaf only for rows of a set that lists a query which uses it (the gate of the regex conditions).  So
 * an exponent literal makes a row a fallback row only if such a condition sits on its leaf - unlike bsg_match_rows_many_range, where
 * ANY range condition of the table does.  Rows of a set with no pair are never walked and never fallback rows.
 * BSG_E_UNSUPPORTED before anything is launched: a condition of kind 3, 4 or 5 (the condition named); more than 64 distinct
 * conditions; program depth 64; the query, op, pair and item limits of bsg_match_rows_wide.  BSG_E_INVALID: what bsg_match_rows_wide
 * refuses, a range entry of another length than BSG_RANGE_ENTRY_BYTES or a flag bit above 3 (the condition named), a kind above 6.
 * Fallback rows, only among rows of a set with at least one pair (all their pair bits 0, never counted in a list): the walker's
 * envelope, a fingerprint collision with ANY table condition (a range condition's field included), an exponent literal as above. */
BSG_API int32_t bsg_match_rows_wide_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                          const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                          const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                          const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                          uint32_t n_sets, const bsg_tokenizer *tok,
                                          uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                          uint32_t *out_n_fallback);
BSG_API int32_t bsg_match_rows_wide_range_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                               const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                               const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                               const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                               uint32_t n_sets, const bsg_tokenizer *tok,
                                               uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                               uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                               uint32_t *out_n_fallback);
/* bsg_match_rows_wide / bsg_match_rows_wide_rows with every condition kind allowed in ONE table (kinds 0-6; the storing walkers
 * k_match_rows_store_regex_substr_range*): the parameter lists, sets, pairs and the implicit set, result layouts, bsg_match_wide_size,
 * bsg_match_pair_rows_list, the list passes, sharding, chunked upload and bsg_last_match_ms of the two wide calls.  Pair p's bits = what
 * bsg_match_rows_regex_substr_range returns for the program of set_queries[p] alone over the set's rows, on every row neither call
 * hands back.  The table decides the path, as in bsg_match_rows_regex_substr_range: a table without a range condition is
 * bsg_match_rows_wide_substr(_rows)'s (the same kernels, caps, bits and refusals), one with range conditions and no condition of kind
 * 3, 4 or 5 is bsg_match_rows_wide_range(_rows)'s; any other table is fed by one walk to the DFAs (a number literal raw, as any leaf
 * text), the needles (folded) and the number parser.
 * Gating is the union of the wide parents': a FieldRegex condition opens its DFA, and a FieldRange condition listens, on a leaf only
 * for rows of a set that lists a query which uses it; every needle listens on every walked row; the flag of a condition none of the
 * set's queries references is unspecified; rows of a set with no pair are never walked and never fallback rows.
 * Limits (BSG_E_UNSUPPORTED before anything is launched, the condition named): 64 distinct conditions; 16 distinct regex conditions
 * with patterns in the compiler's subset; regex tables of at most 42 496 bytes of LDS, whether or not the table holds a needle (the
 * needle table is always there: 39 424 bytes and three workgroups per CU without regex tables, 80 KiB and two with them); a needle of
 * at most 64 bytes after folding, the needles packed first-fit in condition order into 2 words of 64 bytes; program depth 64; the
 * query, op, pair and item limits of bsg_match_rows_wide.  BSG_E_INVALID: what bsg_match_rows_wide refuses, a kind above 6, a range
 * entry of another length than BSG_RANGE_ENTRY_BYTES or a flag bit above 3 (the condition named), an empty needle or one that is not
 * valid UTF-8.
 * Fallback rows, only among rows of a set with at least one pair (all their pair bits 0, never counted in a list): the union of the
 * parents' rules — the walker's envelope, a fingerprint collision with ANY table condition, more than 4 regex conditions of the set's
 * queries on one leaf, a rune the lower table cannot decide, an exponent literal on a leaf where a range condition used by the set's
 * queries listens (bsg_match_rows_wide_range's rule, not bsg_match_rows_many_regex_substr_range's "any range condition of the table"). */
BSG_API int32_t bsg_match_rows_wide_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                       const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                       const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                       const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                                       uint32_t n_sets, const bsg_tokenizer *tok,
                                                       uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                       uint32_t *out_n_fallback);
BSG_API int32_t bsg_match_rows_wide_regex_substr_range_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                            const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                            const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                                            uint32_t n_sets, const bsg_tokenizer *tok,
                                                            uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                                            uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                            uint32_t *out_n_fallback);
/* One pair of bsg_match_rows_wide_rows, whatever its tag, as its ascending set-relative row indices (host arithmetic without a
 * context): payload = out_payload + out_pair_off[p] (not read for NONE / ALL), set_rows = the rows of the pair's set.  *out_n is the
 * full count; at most cap indices are written.  BSG_E_INVALID: a header and payload that are no pair of such a set (a count the
 * tag's rule excludes, indices that do not ascend below set_rows, DENSE bits past the last row). */
BSG_API int32_t bsg_match_pair_rows_list(uint32_t hdr, const uint32_t *payload, uint32_t set_rows, uint32_t *out_rows, uint32_t cap,
                                         uint32_t *out_n);
/* bsg_match_rows_wide / bsg_match_rows_wide_rows over a table of up to BSG_MATCH_LOOKUP_MAX_CONDS distinct conditions: a batch of
 * standing searches has about as many distinct tokens as queries, and cut into tables of 64 conditions it uploads and walks the same
 * rows once per table.  The arguments and the results are exactly those of the two wide calls: sets, pairs and the implicit set, tok,
 * sharding at set-relative multiples of 64 rows, chunked upload, the fallback-row rules, the canonical tagged lists,
 * bsg_match_wide_size and bsg_match_pair_rows_list.  For a table both hold, the results are equal word for word, header for header,
 * fallback row for fallback row.
 * What differs: the walker (k_match_rows_lookup*) resolves every emission by a hash lookup instead of comparing it with every
 * condition, and keeps ceil(n_conds / 64) flag words per row, which k_eval_row_programs_w evaluates the programs over.
 * Condition kinds: Field, Token and FieldToken only.  A BSG_KIND_FIELD_REGEX condition is BSG_E_UNSUPPORTED (the message names the
 * condition): batches with regex conditions take bsg_match_rows_lookup_regex or bsg_match_rows_wide.  A condition repeated in the
 * table is decided once.
 * Limits (BSG_E_UNSUPPORTED before anything is launched): 1 024 conditions; program depth 64; the query, op, pair and item limits of
 * bsg_match_rows_wide.  Device memory: 8 * ceil(n_conds / 64) + 1 bytes per row for the flags and the state byte, 4 per lowered op,
 * query and pair, 8 per result word, at most 48 KiB of tables.
 * bsg_last_match_ms as after the wide call of the same shape. */
#define BSG_MATCH_LOOKUP_MAX_CONDS 1024u
BSG_API int32_t bsg_match_rows_lookup(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                      const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                      const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                      const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                      uint32_t n_sets, const bsg_tokenizer *tok,
                                      uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                      uint32_t *out_n_fallback);
BSG_API int32_t bsg_match_rows_lookup_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                           const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                           const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                           uint32_t n_sets, const bsg_tokenizer *tok,
                                           uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                           uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                           uint32_t *out_n_fallback);
/* bsg_match_rows_lookup / bsg_match_rows_lookup_rows with BSG_KIND_FIELD_REGEX conditions allowed in the table, as
 * bsg_match_rows_many_regex is to bsg_match_rows_many: the same arguments, the same results.  A table without a regex condition runs
 * the same kernels as the two calls above and returns the same bytes.
 * The regex conditions are matched as by bsg_match_rows_wide (patterns in the DFA compiler's subset, the leaf's candidate text, a
 * condition on field f sees the leaves at f or under f + "."): a leaf opens a condition's DFA only on rows of a set that lists a
 * query whose program references it, and a row on which more than 4 such conditions lie on one leaf is a fallback row.  A regex
 * condition repeated in the table (the same field and pattern bytes) is one condition.
 * Limits (BSG_E_UNSUPPORTED before anything is launched), beyond those of bsg_match_rows_lookup: 16 distinct regex conditions; a
 * pattern outside the subset (the message names the condition and the pattern); regex tables of more than
 * 81 920 - (4 * string slots + 8 * pair slots + 29 696) bytes, where the slots are the least powers of two >= 2 * the table's
 * distinct role strings / FieldToken pairs (at least 2): 52 200 bytes over a table of regex conditions only, 19 456 over one with
 * 2 048 strings and 1 024 pairs.  The message names the cap of the table given. */
BSG_API int32_t bsg_match_rows_lookup_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                            const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                            const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                            uint32_t n_sets, const bsg_tokenizer *tok,
                                            uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                            uint32_t *out_n_fallback);
BSG_API int32_t bsg_match_rows_lookup_regex_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                 const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                 const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                 const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                                 uint32_t n_sets, const bsg_tokenizer *tok,
                                                 uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap,
                                                 uint64_t *out_payload_len, uint32_t *out_fallback_rows, uint32_t fallback_cap,
                                                 uint32_t *out_n_fallback);
/* ---- Bucketed hit counts: per (set, query) pair, how many matching rows fall into each bucket of a number field ----
 * bsg_match_rows_wide_regex_substr_range with a third result policy next to "words" and "rows": the condition table (kinds 0-6),
 * programs, sets, pairs and the implicit set, tok, the limits, the refusals and the table-decides-the-walker routing are that call's,
 * and so are the walk and the evaluation (the same kernels).  Instead of bit rows the call returns, per pair p,
 * BSG_HIST_SLOTS(n_buckets) u32 at out_counts[p * BSG_HIST_SLOTS(n_buckets)]: slots [0, B) the buckets, B below, B + 1 above,
 * B + 2 missing.
 * The field and the row's value: a TOP-LEVEL key of 1 to BSG_MINMAX_MAX_NAME bytes by the rule of the per-set MinMax indexes (compared
 * byte for byte with the decoded key; the value must itself be a JSON number; the last member with the key counts); t is the `min`
 * half of that contract, clamp(floor(v)) of the exact decimal value in int64.
 * The bucket rule, in exact integer arithmetic: t < origin is `below`; else d = (uint64_t)t - (uint64_t)origin, q = d / width;
 * q >= n_buckets is `above`, else bucket q.  A row with no such member, or whose last such member is no number, is `missing`.
 * A pair's slots count exactly the rows whose bit bsg_match_rows_wide_regex_substr_range sets for the pair, so they sum to that bit
 * row's popcount minus the rows this call hands back beyond the parent's.
 * Rows handed back: ONE list, ascending, each row once, counted in no slot, only rows of a set with at least one pair: the union of
 * the parent's rules and the bucket scanner's undecided rows (an exponent literal on the field, a backslash in any top-level key).
 * The host decides both the match and the bucket of such a row (bsh_hist_row, bloomsearch_host.h).  Rows of a set with no pair are
 * never scanned, never walked and never handed back.
 * BSG_E_INVALID, before anything is launched and naming the argument: n_buckets 0 or above BSG_HIST_MAX_BUCKETS, width 0, a name
 * that is empty or longer than BSG_MINMAX_MAX_NAME, a null array, and everything the parent refuses.  BSG_E_UNSUPPORTED: as the
 * parent.  n_rows == 0 or zero pairs: BSG_OK, nothing written.
 * Kernels (hist.hip.h): k_bucket_rows / k_bucket_rows_sets beside every chunk's walk, one lane per row, a u16 code per row;
 * k_pair_hist behind k_eval_row_programs, a wave per (pair, span of tiles) with a histogram of BSG_HIST_SLOTS(1024) u32 in LDS, four
 * waves per workgroup: 16 432 bytes.  Device memory beyond the parent's: 2 bytes per row (and 4 for the scanner's list) and
 * 4 * BSG_HIST_SLOTS(n_buckets) per pair of the part; index arithmetic over pairs x slots is in 64 bits.
 * Sharding and chunked upload as the parent: a set cut between devices has its counts added on the host, so the result is the same
 * for any number of devices and any chunk size.  bsg_last_match_ms: the walk plus the evaluation, as after the parent.
 * The lookup family (bsg_match_rows_lookup*) has no such call yet. */
#define BSG_HIST_MAX_BUCKETS 1024u
#define BSG_HIST_SLOTS(n_buckets) ((n_buckets) + 3u)   /* [0, B): buckets, B: below, B + 1: above, B + 2: missing */
BSG_API int32_t bsg_match_rows_wide_hist(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                         const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                         const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                         const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries,
                                         uint32_t n_sets, const bsg_tokenizer *tok,
                                         const uint8_t *field, uint32_t field_len, int64_t origin, uint64_t width, uint32_t n_buckets,
                                         uint32_t *out_counts /* [n_pairs * BSG_HIST_SLOTS(n_buckets)] */,
                                         uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback);
/* the bucket scanner (summed over chunks) + the counting pass of the most recent bsg_match_rows_wide_hist, slowest device */
BSG_API int32_t bsg_last_hist_ms(bsg_ctx *ctx, float *hist_ms);
/* Device time of the most recent k_match_rows / k_match_rows_regex / k_match_rows_many / k_match_rows_many_regex dispatch (the
 * slowest device's); after bsg_match_rows_wide, its walk plus its evaluation; after bsg_match_rows_wide_rows, its list passes too. */
BSG_API int32_t bsg_last_match_ms(bsg_ctx *ctx, float *match_ms);

#ifdef __cplusplus
}
#endif
#endif /* BLOOMGPU_H */
