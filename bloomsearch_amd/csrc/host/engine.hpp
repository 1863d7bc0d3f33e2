// engine.hpp — host-side mirror of the reference's BloomSearchEngine surface for THIS path only:
//   IngestRows  (ingest.go:170, processIngestRequest :330-531: partitioning, whole-batch validation,
//                indexRow into per-partition bloomEntrySets, flush triggers)
//   Flush       (ingest.go:197; handleFlush flush.go:138-282: per partition buffer buildFilters ->
//                encodeFilterSection; unionInto(fileEntries); file-level buildFilters; counts stamped)
//   Query       (query_exec.go:201-444: file stage over file-level filters, evaluateBlockFilters per
//                candidate block with BloomFilterSkipped stats, final matchRowBytes scan)
//   Merge       (merge.go:440-817 rebuild semantics: re-index every row, right-size, never OR)
// The bloom arithmetic AND both directions of the filter-section codec run on the GPU through the C-ABI
// (bsg_build_sections / bsg_ingest_* / bsg_arena_load_sections / bsg_probe);
// there is no CPU bloom path here.  Storage, compression, durability, goroutines and the
// DataStore / MetaStore plugins are out of scope: "files" are kept in memory with the reference's
// filter-section bytes (section_codec.hpp) so the wire layout is exercised end to end.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <tuple>
#include <vector>

#include "bloomgpu.h"
#include "entry_sets.hpp"
#include "expression.hpp"
#include "regex_groups.hpp"
#include "section_codec.hpp"
#include "range.hpp"
#include "range_text_groups.hpp"
#include "minmax.hpp"
#include "substring.hpp"
#include "substring_groups.hpp"
#include "wide_plan.hpp"
#include "lookup_plan.hpp"

namespace bsh {

enum EngineError : int32_t {
    kEngineOk = 0,
    kErrInvalidConfig = -101,   // ErrInvalidConfig (engine.go:16-34)
    kErrEngineStopped = -102,   // ErrEngineStopped
    kErrInvalidRow = -103,      // a row of the batch is not a JSON object: whole batch rejected (ingest.go:378-397)
    kErrInvalidQuery = -104,
    kErrGpu = -105,             // a bsg_* call failed (message carries bsg_last_error)
    kErrInvalidHash = -106,     // ErrInvalidHash: filter section CRC mismatch
};

struct EngineConfig {           // BloomSearchEngineConfig (engine.go:82-147), the knobs on this path
    uint64_t max_row_group_rows = 10000;
    uint64_t max_row_group_bytes = 10ull * 1024 * 1024;
    uint64_t max_buffered_rows = 1000;
    uint64_t max_buffered_bytes = 1ull * 1024 * 1024;
    double bloom_false_positive_rate = 0.001;
    std::string partition_field;  // PartitionFunc stand-in: top-level key whose text is the partition id ("" = none)
    // true: rows are only validated and buffered at ingest; walking, tokenizing, dedup, counting and the filter
    // build all run on the device at flush / merge time (bsg_ingest_*), the host walker only finishing the rows
    // the device walker hands back.  false: indexRow on the host at ingest time, as the reference does.
    bool device_ingest = false;
    // true (with device_ingest; alone it is an invalid config): every validated ingest_rows batch is handed to an open streaming
    // ingest when it arrives (bsg_ingest_open / bsg_ingest_add_sets / bsg_ingest_append_rows: one set per partition buffer, the
    // file as their only parent) and the rows it hands back are finished by the host walker at once; flush only finishes, sizes
    // and builds.  Merge keeps the one-shot path.  Off by default.
    bool device_ingest_stream = false;
    // true: the caller promises that every row is one valid JSON object (the reference marshals its own rows, ingest.go:379-396):
    // ingest_rows validates no row for its own sake (a partition id is still found where a PartitionField asks for one).
    bool trusted_rows = false;
    // true (needs device_ingest_stream, trusted_rows and a partition_field of 1 to 64 bytes; anything else is an invalid config): the
    // batches go to a KEYED streaming ingest (bsg_ingest_open_keyed / bsg_ingest_append_rows_keyed): the device finds every row's
    // partition text, and validate_object_row runs only over the rows it hands back.  Off by default.
    bool device_partition = false;
    // true: the final row test of the surviving blocks (matchRowBytes, query_exec.go:751) runs on the device too
    // (bsg_match_rows); rows it hands back, and expressions beyond its limits, go through the host matcher.
    bool device_match = false;
    // true (with device_match): queries whose regex patterns all compile to the device's byte DFAs (regex_dfa.hpp) are
    // matched bloom AND regex by ONE bsg_match_rows_regex call, and the rows it hands back by the host matcher with the same
    // DFAs (RE2 semantics on both sides); other regex queries keep the std::regex path below.  Off by default.
    bool device_regex = false;
    // true (with device_match): query() decides a query that has a Range tree beside a Regex and / or a Substring tree by ONE
    // bsg_match_rows_regex_substr_range call over And(bloom root | TRUE, regex root, substring root, range root).  A regex tree takes
    // part only under device_regex with every pattern in the device subset; otherwise it is left out of the call (TRUE in its place),
    // range and substring are still decided in the one call, and the host regex matcher filters the hits (with no substring tree
    // either there is nothing to put beside the range: the route without the key).  The rows the call hands back are decided by the
    // host matchers together; BSG_E_UNSUPPORTED from the library means the route without the key, and only that route's calls are
    // counted.  With no wide or lookup key set, query_many lets range conditions and text conditions share a group, decided by ONE
    // bsg_match_rows_many_regex_substr_range call (range_text_groups.hpp: the closing rules, and the reduced 34 032-byte cap of the
    // regex tables as soon as kind 6 sits beside a text condition); under a wide or lookup key groups never mix (range_groups.hpp
    // joins) and such a query goes to query(), unless device_match_range_text_wide is set as well.  Off by default: every route and every counted entry point is then exactly what it is
    // without the key.
    bool device_match_range_text = false;
    // true (needs device_match, device_match_range_text and at least one of the wide or lookup keys below; anything else is an invalid
    // config): under those keys query_many lets range and text conditions share a wide group too (range_text_groups.hpp wide_fits: no
    // member limit, 64 conditions, 16 regex conditions, co_active_bound, needles that pack, regex tables of at most 42 496 bytes needle
    // or not), decided by ONE bsg_match_rows_wide_regex_substr_range call - under device_match_wide_rows / device_match_lookup_rows by
    // its _rows twin, the lists consumed as the other wide groups' are.  Under a lookup key such a group is a 64-condition wide group,
    // never a lookup call.  The rows the call hands back are decided by the four host matchers together; BSG_E_UNSUPPORTED sends the
    // group's queries to query(), and the refused call is not counted.  query() is unchanged.  Off by default: every route and every
    // counted entry point is then exactly what it is without the key.
    bool device_match_range_text_wide = false;
    // true (with device_match): query_many packs its queries into groups bounded by the condition table alone (64 distinct
    // conditions, 16 regex conditions, the table bytes, co_active_bound) - not by 64 members - and decides each group by ONE
    // bsg_match_rows_wide call, every set's query list read straight from the probe's survivors (a group that holds a substring
    // condition: ONE bsg_match_rows_wide_substr call, its needles packed and its regex tables under the cap beside them; a group that
    // holds a range condition: ONE bsg_match_rows_wide_range call).  Off by default: routing is then exactly the batched calls'.
    bool device_match_wide = false;
    // true (with device_match): the grouping of device_match_wide, each group decided by ONE bsg_match_rows_wide_rows call: every
    // pair's matching rows come back as a list (or NONE / ALL / its words) and are consumed as such, no bit row is scanned.  Off by
    // default like device_match_wide.
    bool device_match_wide_rows = false;
    // true (with device_match): query_many's groups WITHOUT a regex condition hold up to 1 024 distinct conditions and are each decided
    // by ONE bsg_match_rows_lookup call (device_match_lookup_rows: bsg_match_rows_lookup_rows, the lists consumed as under
    // device_match_wide_rows); a query with a regex condition keeps the 64-condition groups of the wide call, and so does one with a
    // substring or a range condition (the lookup calls take neither).  Off by default.
    bool device_match_lookup = false;
    bool device_match_lookup_rows = false;
    // with either of the two (and device_regex): a group that holds regex conditions keeps the 1 024-condition bound and is decided by
    // ONE bsg_match_rows_lookup_regex(_rows) call; it closes at 16 regex conditions, at more than 4 of them on one leaf, and where
    // their tables pass what the group's strings and pairs (by their upper bounds) leave of the walker's LDS
    bool device_match_lookup_regex = false;
    // true (with device_match and one of device_match_wide / device_match_wide_rows): in query_many the queries that carry a histogram
    // spec form wide groups of their own, one family of groups per distinct spec, closed by the wide groups' rules; each group is
    // decided by ONE bsg_match_rows_wide_hist call, the per-set counts summed per query on the host, the rows it hands back matched and
    // bucketed on the host.  BSG_E_UNSUPPORTED (and every query outside a group) takes the host route: matched as before, bucketed by
    // hist_row_slot.  Off by default; query() always takes the host route.
    bool device_match_histogram = false;
    // Tokenizer (engine.go:83, "for both indexing and verification"), restricted to the separator family
    // strings.FieldsFunc(lower ? strings.ToLower(v) : v, isSep) (text.hpp Tokenizer): indexRow, the host matcher and the
    // device calls (bsg_ingest_rows_tok / bsg_match_rows_tok) all use it.  Default: BasicWhitespaceLowerTokenizer.
    Tokenizer tokenizer;
    // MinMaxIndexes (engine.go: BloomSearchEngineConfig.MinMaxIndexes): top-level keys whose per-block [min, max] every flush records
    // (minmax.hpp; bloomgpu.h "per-set MinMax indexes" for the limits: 1 to 8 distinct names of 1 to 64 bytes, or none).  Without
    // DeviceIngest every row is folded on the host at ingest time; with it the flush's device call computes the indexes
    // (bsg_ingest_rows_minmax / bsg_ingest_open_minmax) and only the rows it hands back are folded on the host.
    std::vector<std::string> minmax_indexes;
};

struct DataBlock {
    std::map<std::string, bsg_minmax> minmax;    // DataBlockMetadata.MinMaxIndexes: the fields some row of the block contributed to
    std::string partition_id;
    std::vector<std::string> rows;
    uint64_t row_bytes = 0;              // uncompressed row bytes incl. the 4-byte length prefixes
    uint64_t block_offset = 0;           // RowDataOffset within the (virtual) file
    BloomEntryCounts counts;             // DataBlockMetadata.BloomEntryCounts (file_format.go:753-757)
    double fpr = 0;
    std::vector<uint8_t> filter_section; // encodeFilterSection bytes
};

struct DataFile {
    uint64_t file_id = 0;
    std::vector<DataBlock> blocks;
    BloomEntryCounts counts;
    std::vector<uint8_t> filter_section; // file-level filters
    // The file's block filters as a resident probe arena live in the LIBRARY's file-arena cache (bsg_file_arena_*, keyed by
    // file_id): published by the flush / merge that built them on the device, or decoded from the stored sections by the first
    // query that misses; least recently used files leave when the byte budget is exceeded, a merged-away file is forgotten.
};

struct BlockStats {                      // query_exec.go:63-72
    uint64_t file_id = 0, block_offset = 0;
    int64_t rows_processed = 0, bytes_processed = 0, total_rows = 0, total_bytes = 0;
    // query_exec.go:578,598-600: the reference timestamps every block; a batched probe has one wall time for all of them,
    // so every candidate block gets batch time / blocks (plus its share of the scan), never zero
    // (query_handles_test.go:1062 asserts Duration > 0)
    int64_t duration_ns = 0;
    bool bloom_filter_skipped = false;
};

// "Histogram" of a query: the bucket spec of bsg_match_rows_wide_hist (field 1 to 64 bytes, width >= 1, 1 to 1 024 buckets)
struct HistSpec {
    std::string field;
    int64_t origin = 0;
    uint64_t width = 1;
    uint32_t buckets = 1;
    bool operator<(const HistSpec &o) const { return std::tie(field, origin, width, buckets) < std::tie(o.field, o.origin, o.width, o.buckets); }
};

struct QueryResult {
    std::vector<uint64_t> hist;          // buckets + 3 counts where the device route decided a histogram query (rows is then empty)
    std::vector<std::string> rows;
    std::vector<BlockStats> block_stats;
    std::vector<std::string> errors;     // per-block failures joined into Results.Err by the reference
    uint64_t files_considered = 0, files_bloom_skipped = 0;
};

class BloomSearchEngine {
public:
    BloomSearchEngine(const EngineConfig &cfg, bsg_ctx *ctx) : cfg_(cfg), ctx_(ctx) {}
    ~BloomSearchEngine() { drop_stream(); drop_arenas(); }

    static int32_t validate(const EngineConfig &c, std::string &err)
    {
        if (c.max_row_group_rows == 0 || c.max_row_group_bytes == 0) { err = "MaxRowGroupRows / MaxRowGroupBytes must be positive"; return kErrInvalidConfig; }
        if (!(c.bloom_false_positive_rate > 0.0 && c.bloom_false_positive_rate < 1.0)) { err = "BloomFalsePositiveRate must be in (0, 1)"; return kErrInvalidConfig; }
        if (c.device_ingest_stream && !c.device_ingest) { err = "DeviceIngestStream needs DeviceIngest"; return kErrInvalidConfig; }
        if (c.device_partition && !c.device_ingest_stream) { err = "DevicePartition needs DeviceIngestStream"; return kErrInvalidConfig; }
        if (c.device_partition && !c.trusted_rows) { err = "DevicePartition needs TrustedRows"; return kErrInvalidConfig; }
        if (c.device_partition && (c.partition_field.empty() || c.partition_field.size() > BSG_PARTITION_MAX_NAME)) {
            err = "DevicePartition needs a PartitionField of 1 to 64 bytes";
            return kErrInvalidConfig;
        }
        if (c.device_match_range_text_wide && !(c.device_match && c.device_match_range_text &&
                                                (c.device_match_wide || c.device_match_wide_rows || c.device_match_lookup || c.device_match_lookup_rows))) {
            err = "DeviceMatchRangeTextWide needs DeviceMatch, DeviceMatchRangeText and one of DeviceMatchWide, DeviceMatchWideRows, DeviceMatchLookup, DeviceMatchLookupRows";
            return kErrInvalidConfig;
        }
        if (c.device_match_histogram && !(c.device_match && (c.device_match_wide || c.device_match_wide_rows))) {
            err = "DeviceMatchHistogram needs DeviceMatch and one of DeviceMatchWide, DeviceMatchWideRows";
            return kErrInvalidConfig;
        }
        if (!c.minmax_indexes.empty() && !MinMaxFieldNames::check(c.minmax_indexes, err)) { err = "MinMaxIndexes: " + err; return kErrInvalidConfig; }
        return kEngineOk;
    }

    const std::string &last_error() const { return err_; }
    // how often the engine has called each device row-matcher entry point (bsg_match_rows_*), by name: which route its queries took
    std::map<std::string, uint64_t> match_calls() const
    {
        std::lock_guard<std::mutex> lk(match_calls_mu_);
        return match_calls_;
    }
    // DeviceIngestStream at work (bse_describe "IngestStream"): batches and rows handed to a streaming ingest at ingest time, the
    // rows among them the host walker finished at once, and the flushes built from a stream (not from the kept row bytes)
    struct StreamStats { uint64_t batches = 0, rows = 0, host_rows = 0, flushes = 0; };
    const StreamStats &stream_stats() const { return stream_stats_; }
    const std::vector<DataFile> &files() const { return files_; }

    void stop() { stopped_ = true; }

    // Fault injection (the reference's tests use corrupting DataStore doubles): flip one byte of a stored section.
    bool corrupt_section_byte(size_t file_index, int block_index, size_t byte_index)
    {
        if (file_index >= files_.size()) return false;
        std::vector<uint8_t> *sec = &files_[file_index].filter_section;
        if (block_index >= 0) {
            if ((size_t)block_index >= files_[file_index].blocks.size()) return false;
            sec = &files_[file_index].blocks[block_index].filter_section;
        }
        if (byte_index >= sec->size()) return false;
        (*sec)[byte_index] ^= 0x5A;
        if (block_index >= 0) forget_file_arena(files_[file_index]);   // re-read (and re-checked) from the stored bytes on next use
        else drop_files_arena();
        return true;
    }

    // rows: one marshaled JSON object per element.  Whole batch is validated before any buffer
    // is touched (ingest.go:378-397).
    int32_t ingest_rows(const std::vector<std::string_view> &rows)
    {
        if (stopped_) return fail(kErrEngineStopped, "engine stopped");
        if (rows.empty()) return kEngineOk;  // ingest.go:356-359
        std::vector<std::string> pids(rows.size());
        std::string scratch;
        // DevicePartition: the device finds the partition ids (stream_append_keyed fills pids); TrustedRows without a PartitionField:
        // nothing is asked of a row here
        const bool keyed = cfg_.device_partition && !stream_broken_;
        const bool skip = keyed || (cfg_.trusted_rows && cfg_.partition_field.empty());
        for (size_t i = 0; i < rows.size() && !skip; ++i) {
            bool has_pid = false;
            if (!validate_object_row(rows[i], cfg_.partition_field, pids[i], has_pid, scratch))
                return fail(kErrInvalidRow, "row " + std::to_string(i) + " is not a JSON object");
            if (!has_pid) pids[i].clear();
        }
        // the batch goes to the device now.  A failure is the caller's to see, like the one-shot path's at flush: the batch is not
        // buffered, the stream is dropped, and the rows buffered so far are built from their kept bytes (build_sections_device).
        if (cfg_.device_ingest_stream && !stream_broken_) {
            if (int32_t rc = keyed ? stream_append_keyed(rows, pids) : stream_append(rows, pids)) { drop_stream(); stream_broken_ = true; return rc; }
        }
        bool should_flush = false;
        for (size_t i = 0; i < rows.size(); ++i) {
            PartitionBuffer &pb = buffers_[pids[i]];
            pb.entries.tok = cfg_.tokenizer;
            if (!cfg_.device_ingest) pb.entries.index_row(rows[i]);   // HOT: walk + tokenize + dedup (ingest.go:450)
            if (!cfg_.device_ingest && !cfg_.minmax_indexes.empty()) {   // ingest.go:455-470; under DeviceIngest the flush's device call does it
                pb.minmax.resize(cfg_.minmax_indexes.size(), bsg_minmax{});
                minmax_row(rows[i], cfg_.minmax_indexes, pb.minmax.data());
            }
            pb.rows.emplace_back(rows[i]);
            pb.bytes += rows[i].size() + 4;
            buffered_rows_ += 1;
            buffered_bytes_ += rows[i].size() + 4;
            if (pb.rows.size() >= cfg_.max_row_group_rows || pb.bytes >= cfg_.max_row_group_bytes) should_flush = true;
        }
        if (buffered_rows_ >= cfg_.max_buffered_rows || buffered_bytes_ >= cfg_.max_buffered_bytes) should_flush = true;
        return should_flush ? flush() : kEngineOk;
    }

    // handleFlush: one file, one data block per partition buffer, all filters built in ONE bsg_build call.
    int32_t flush()
    {
        if (buffers_.empty()) return kEngineOk;
        DataFile file;
        file.file_id = next_file_id_++;
        BloomEntrySets file_entries;
        std::vector<const BloomEntrySets *> sets;
        for (auto &kv : buffers_) {
            DataBlock blk;
            blk.partition_id = kv.first;
            blk.rows = std::move(kv.second.rows);
            blk.row_bytes = kv.second.bytes;
            blk.fpr = cfg_.bloom_false_positive_rate;
            if (!cfg_.device_ingest) {
                blk.counts = kv.second.entries.counts();
                kv.second.entries.union_into(file_entries);   // flush.go:221
                set_block_minmax(blk, kv.second.minmax.data(), kv.second.minmax.size());
            }
            file.blocks.push_back(std::move(blk));
        }
        std::vector<std::vector<uint8_t>> sections;
        bool minmax_done = !cfg_.device_ingest || cfg_.minmax_indexes.empty();
        if (cfg_.device_ingest_stream && stream_ && !stream_broken_) {
            if (int32_t rc = build_sections_stream(file, sections, minmax_done)) return rc;
            stream_stats_.flushes += 1;
        } else if (cfg_.device_ingest) {
            if (int32_t rc = build_sections_device(file, sections, &minmax_done)) return rc;
        } else {
            for (auto &kv : buffers_) sets.push_back(&kv.second.entries);
            sets.push_back(&file_entries);                    // file-level filters sized for the union (flush.go:253)
            if (int32_t rc = build_sections(sets, sections)) return rc;
            file.counts = file_entries.counts();
        }
        if (!minmax_done) host_minmax_blocks(file);          // a flush that fell back to the host walker for its sets
        uint64_t off = 0;
        for (size_t b = 0; b < file.blocks.size(); ++b) {
            file.blocks[b].filter_section = std::move(sections[b]);
            file.blocks[b].block_offset = off;
            off += file.blocks[b].row_bytes;
        }
        file.filter_section = std::move(sections.back());
        files_.push_back(std::move(file));
        buffers_.clear();
        buffered_rows_ = buffered_bytes_ = 0;
        drop_stream();               // the next batch opens the next one
        stream_broken_ = false;
        drop_files_arena();          // one more file-level "block"; the other files' block arenas stay where they are
        return kEngineOk;
    }

    // Merge (merge.go rebuild semantics): every source row is re-walked into fresh block + file
    // entry sets and filters are rebuilt right-sized; blocks of one partition are merged while they
    // fit MaxRowGroupRows / MaxRowGroupBytes.
    int32_t merge()
    {
        if (files_.size() < 2) return kEngineOk;
        std::map<std::string, std::vector<DataBlock *>> by_partition;
        for (auto &f : files_) for (auto &b : f.blocks) by_partition[b.partition_id].push_back(&b);
        DataFile out;
        out.file_id = next_file_id_++;
        std::vector<std::unique_ptr<BloomEntrySets>> block_sets;
        BloomEntrySets file_entries;
        for (auto &kv : by_partition) {
            DataBlock cur;
            auto start_block = [&]() { cur = DataBlock{}; cur.partition_id = kv.first; cur.fpr = cfg_.bloom_false_positive_rate; block_sets.push_back(std::make_unique<BloomEntrySets>(cfg_.tokenizer)); };
            auto finish_block = [&]() {
                if (!cfg_.device_ingest) {
                    cur.counts = block_sets.back()->counts();
                    block_sets.back()->union_into(file_entries);
                }
                out.blocks.push_back(std::move(cur));
            };
            start_block();
            for (DataBlock *src : kv.second) {
                // merge.go:208-260: two blocks of a partition merge only when their MinMax KEY SETS are equal; the merged index is the
                // union of the sources' (exact under every ingest route: the fold is associative, so nothing is recomputed)
                if (!cur.rows.empty() && (cur.rows.size() + src->rows.size() > cfg_.max_row_group_rows ||
                                          cur.row_bytes + src->row_bytes > cfg_.max_row_group_bytes || !same_minmax_keys(cur, *src))) { finish_block(); start_block(); }
                for (auto &kv2 : src->minmax) minmax_fold(cur.minmax[kv2.first], kv2.second.min, kv2.second.max);
                for (auto &r : src->rows) {
                    if (!cfg_.device_ingest) block_sets.back()->index_row(r);      // merge.go:746
                    cur.row_bytes += r.size() + 4;
                    cur.rows.push_back(std::move(r));
                }
            }
            finish_block();
        }
        std::vector<std::vector<uint8_t>> sections;
        if (cfg_.device_ingest) {
            if (int32_t rc = build_sections_device(out, sections)) return rc;
        } else {
            std::vector<const BloomEntrySets *> sets;
            for (auto &s : block_sets) sets.push_back(s.get());
            sets.push_back(&file_entries);
            if (int32_t rc = build_sections(sets, sections)) return rc;
            out.counts = file_entries.counts();
        }
        uint64_t off = 0;
        for (size_t b = 0; b < out.blocks.size(); ++b) {
            out.blocks[b].filter_section = std::move(sections[b]);
            out.blocks[b].block_offset = off;
            off += out.blocks[b].row_bytes;
        }
        out.filter_section = std::move(sections.back());
        for (auto &f : files_) forget_file_arena(f);    // tombstoned sources (merge.go:178-185)
        files_.clear();
        files_.push_back(std::move(out));
        drop_files_arena();
        return kEngineOk;
    }

    // Query: nil expression => no bloom conditions => no filter reads, every block scanned (query_exec.go:503-508).
    // regex: the field-scoped regex tree of the query; files and blocks are pruned by
    // pruneBloomQuery = AndBloomQueries(bloom, RegexFieldGuardBloomQuery(regex)) (query_exec.go:220), rows are matched by the
    // bloom tree AND the regex tree (row_matcher.go:353-368).
    // sub: the substring tree of the query (substring.hpp).  Its guard over the pruning terms is a third side of the pruning
    // expression, And(bloom, regex field guard, substring guard); the row test is bloom AND regex AND substring.  Under DeviceMatch a
    // query without a regex tree is decided by ONE bsg_match_rows_substr call over the program And(bloom root, substring root) (the
    // rows it hands back: the host matchers).  With a regex tree, under DeviceMatch + DeviceRegex and patterns in the device subset, ONE
    // bsg_match_rows_regex_substr call decides And(bloom root, regex root, substring root); where the library answers
    // BSG_E_UNSUPPORTED (tables over the cap beside the needle table, needles that do not pack) the regex call decides its two sides
    // and SubstringRowMatcher the third, as for every other combination of the keys and without DeviceMatch.
    // range: the range tree of the query (range.hpp).  Its guard — every condition as Field(field) — is a fourth side of the pruning
    // expression; the row test is bloom AND regex AND substring AND range.  Under DeviceMatch a query with neither a regex nor a
    // substring tree is decided by ONE bsg_match_rows_range call over the program And(bloom root, range root) (the rows it hands back,
    // those with an exponent literal on a range field among them: the host matchers).  Every other combination takes the route it
    // took without the range tree, and RangeRowMatcher filters its hits.
    // prefilter: the tree over the blocks' partition ids and MinMax indexes (minmax.hpp); nullptr takes exactly the path without one.
    int32_t query(const BloomExpression *row_expr, QueryResult &out, const RegexExpression *regex = nullptr, const SubstringExpression *sub = nullptr,
                  const RangeExpression *range = nullptr, const PrefilterExpression *prefilter = nullptr)
    {
        out = QueryResult{};
        const auto t_begin = std::chrono::steady_clock::now();
        SubstringRowMatcher sub_matcher(sub, cfg_.tokenizer);
        if (!sub_matcher.valid()) return fail(kErrInvalidQuery, "substring needle: non-empty valid UTF-8 of at most 64 bytes after folding");
        RangeRowMatcher range_matcher(range);
        BloomExpression guard, sub_guard, range_guard_storage, two_storage, three_storage, prune_storage;
        const bool has_guard = regex_field_guard(regex, guard);
        const bool has_two = and_bloom_queries(row_expr, has_guard ? &guard : nullptr, two_storage);
        const bool has_sub_guard = substring_guard(sub, cfg_.tokenizer, sub_guard);
        const bool has_three = and_bloom_queries(has_two ? &two_storage : nullptr, has_sub_guard ? &sub_guard : nullptr, three_storage);
        const bool has_range_guard = range_guard(range, range_guard_storage);
        const BloomExpression *expr = and_bloom_queries(has_three ? &three_storage : nullptr, has_range_guard ? &range_guard_storage : nullptr, prune_storage) ? &prune_storage : nullptr;
        std::vector<Survivors> sv;
        if (int32_t rc = probe_stage({expr}, sv)) return rc;
        apply_prefilter(prefilter, sv[0]);
        const std::vector<uint8_t> &file_ok = sv[0].file_ok;
        const int64_t probe_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
        size_t candidate_blocks = 0;
        for (size_t f = 0; f < files_.size(); ++f) if (file_ok[f]) candidate_blocks += files_[f].blocks.size();
        const int64_t probe_share = candidate_blocks ? std::max<int64_t>(1, probe_ns / (int64_t)candidate_blocks) : 0;
        RowMatcher matcher(row_expr, cfg_.tokenizer);
        RegexRowMatcher regex_matcher(regex);
        RegexRowMatcher regex_dfa(cfg_.device_regex && cfg_.device_match ? regex : nullptr, true);
        const bool regex_on_device = regex && cfg_.device_regex && cfg_.device_match && regex_dfa.valid();
        if (!regex_on_device && !regex_matcher.valid()) return fail(kErrInvalidQuery, "regex pattern does not compile");
        // the scan list: every row of every block that survived both stages, in file / block order
        std::vector<const std::string *> scan;
        std::vector<ScanBlock> scanned;             // the scanned blocks and their block_stats entries (for the scan's time share)
        const auto t_scan = std::chrono::steady_clock::now();
        block_stage_stats(sv[0], probe_share, out, scanned);
        for (const ScanBlock &sb : scanned)
            for (const std::string &row : files_[sb.f].blocks[sb.b].rows) scan.push_back(&row);
        std::vector<uint8_t> hit(scan.size(), 0);
        bool on_device = false, regex_done = false, sub_done = false, range_done = false;
        bool three_done = false;
        const RegexExpression *rx_dev = regex_on_device ? regex : nullptr;     // a regex tree takes part only where the device reads its patterns
        if (cfg_.device_match && cfg_.device_match_range_text && range && (rx_dev || sub) && !scan.empty()) {
            // one walk decides bloom AND regex AND substring AND range; a regex tree left out of it is the host's, below
            if (int32_t rc = match_rows_device_range_text(row_expr, rx_dev, sub, *range, scan, matcher, regex_dfa, sub_matcher, range_matcher, hit, three_done)) return rc;
            if (three_done) { on_device = range_done = true; regex_done = rx_dev != nullptr; sub_done = sub != nullptr; }
        }
        if (range && !regex && !sub && cfg_.device_match && !scan.empty()) {   // one walk decides bloom AND range
            if (int32_t rc = match_rows_device_range(row_expr, *range, scan, matcher, range_matcher, hit, range_done)) return rc;
            on_device = range_done;
        }
        if (regex_on_device && sub && !three_done && !scan.empty()) {      // both trees: one walk decides bloom AND regex AND substring
            bool both_done = false;
            if (int32_t rc = match_rows_device_regex_substr(row_expr, *regex, *sub, scan, matcher, regex_dfa, sub_matcher, hit, both_done)) return rc;
            regex_done = sub_done = both_done;
        }
        if (regex_on_device && !regex_done && !scan.empty()) {
            if (int32_t rc = match_rows_device_regex(row_expr, *regex, scan, matcher, regex_dfa, hit, regex_done)) return rc;
            if (!regex_done && !regex_matcher.valid()) return fail(kErrInvalidQuery, "regex pattern does not compile");
        }
        on_device = on_device || regex_done;
        if (sub && !regex && !three_done && cfg_.device_match && !scan.empty()) {
            if (int32_t rc = match_rows_device_substr(row_expr, *sub, scan, matcher, sub_matcher, hit, sub_done)) return rc;
            on_device = sub_done;
        }
        if (!on_device && cfg_.device_match && row_expr && !scan.empty()) {
            if (int32_t rc = match_rows_device(row_expr, scan, matcher, hit, on_device)) return rc;
        }
        if (!on_device)
            for (size_t i = 0; i < scan.size(); ++i) hit[i] = matcher.match(*scan[i]);
        if (regex && !regex_done) {
            // the regex patterns only run on rows the bloom tree kept AND — when the device matcher is on — on rows whose
            // guard fields exist: the field guard the probe already used, evaluated per row by k_match_rows.  Only when every
            // regex node translated into the guard (regex_guard_is_exact): the reference prunes files and blocks with it, never rows
            std::vector<uint8_t> cand(scan.size(), 1);
            bool guard_on_device = false;
            if (cfg_.device_match && has_guard && regex_guard_is_exact(*regex) && !scan.empty()) {
                RowMatcher guard_host(&guard, cfg_.tokenizer);
                if (int32_t rc = match_rows_device(&guard, scan, guard_host, cand, guard_on_device)) return rc;
                if (!guard_on_device) std::fill(cand.begin(), cand.end(), 1);
            }
            for (size_t i = 0; i < scan.size(); ++i)
                if (hit[i]) hit[i] = cand[i] && regex_matcher.match(*scan[i]);
        }
        if (sub && !sub_done)
            for (size_t i = 0; i < scan.size(); ++i)
                if (hit[i]) hit[i] = sub_matcher.match(*scan[i]);
        if (range && !range_done)
            for (size_t i = 0; i < scan.size(); ++i)
                if (hit[i]) hit[i] = range_matcher.match(*scan[i]);
        for (size_t i = 0; i < scan.size(); ++i)
            if (hit[i]) out.rows.push_back(*scan[i]);
        add_scan_time(t_scan, scanned, out);
        return kEngineOk;
    }

    // A batch of queries in one pass: element i of `results` is what query(exprs[i], ..., regexes[i]) returns (duration_ns aside).
    // One QueryBatch holds every bloom-only query: one file-stage probe, one bsg_probe_many over the leased arenas; the scan list
    // is the rows of every block at least one query survived on, one set per block with its query mask, and - under DeviceMatch -
    // one bsg_match_rows_many call per group of <= 64 queries / <= 64 distinct conditions decides them (the rows it hands back: the
    // host matcher, per query whose mask bit is set).  Without DeviceMatch the host matcher runs per (query, surviving block).
    // A query with a regex tree stays in the batch under DeviceMatch + DeviceRegex when all its patterns compile in the device
    // subset (the test query() makes): it is probed with query()'s pruning expression And(bloom, field guard) and matched as the
    // program And(bloom root | TRUE, regex root) by bsg_match_rows_many_regex.  Every other regex query is answered by query() and
    // placed at its position, and so is a batched one whose group the device did not decide.
    // A query with a substring tree (subs[i]) stays in the batch under DeviceMatch when its needles are valid (and, with a regex tree as
    // well, under the regex rule above): it is probed with query()'s pruning expression And(bloom, regex field guard, substring guard)
    // and matched as the program And(bloom root | TRUE, regex root, substring root) in its group's call — bsg_match_rows_many_substr /
    // bsg_match_rows_many_regex_substr, or bsg_match_rows_wide_substr(_rows) under the wide keys (substring_groups.hpp says when a
    // group closes and which call it makes).  Every other substring query is answered by query(), and so is a batched one whose
    // group the device did not decide.
    // A query with a range tree (ranges[i]) and neither a regex nor a substring tree stays in the batch under DeviceMatch: it is probed
    // with query()'s pruning expression And(bloom, range guard) and matched as the program And(bloom root | TRUE, range root) in its
    // group's call — bsg_match_rows_many_range, or bsg_match_rows_wide_range(_rows) under the wide and the lookup keys
    // (range_groups.hpp: a group never holds a range condition beside a regex or substring one).  A range query with one of the other two
    // trees, every range query without DeviceMatch, and a batched one whose group the device did not decide are answered by query().
    // Under DeviceMatchRangeText with no wide or lookup key, a range query WITH a regex and / or substring tree stays in the batch (by
    // the rules above for those trees): it is probed with And(bloom, regex field guard, substring guard, range guard), its program is
    // And(bloom root | TRUE, its trees), and a group whose table holds kind 6 beside a kind 3-5 condition makes ONE
    // bsg_match_rows_many_regex_substr_range call (range_text_groups.hpp).  Under a wide or lookup key the same holds with
    // DeviceMatchRangeTextWide as well: the mixed group is a wide group and makes ONE bsg_match_rows_wide_regex_substr_range(_rows) call.
    int32_t query_many(const std::vector<const BloomExpression *> &exprs, const std::vector<const RegexExpression *> &regexes,
                       std::vector<QueryResult> &results, const std::vector<const SubstringExpression *> *subs = nullptr,
                       const std::vector<const RangeExpression *> *ranges = nullptr, const std::vector<const PrefilterExpression *> *prefilters = nullptr,
                       const std::vector<const HistSpec *> *hists = nullptr)
    {
        // every query has its own prefilter mask on its survivors: a block no query of the batch keeps is never walked
        auto prefilter_of = [&](size_t i) { return prefilters && i < prefilters->size() ? (*prefilters)[i] : nullptr; };
        results.assign(exprs.size(), QueryResult{});
        const bool mix_ok = bsh_rtg::mixing(cfg_.device_match, cfg_.device_match_range_text, any_wide_key()) ||
                            bsh_rtg::wide_mixing(cfg_.device_match, cfg_.device_match_range_text, cfg_.device_match_range_text_wide, any_wide_key());
        std::vector<size_t> live;                   // the batch: queries without a regex tree, and regex queries the device matches
        std::vector<const RegexExpression *> live_regex;
        std::vector<const SubstringExpression *> live_sub;
        std::vector<const RangeExpression *> live_range;
        std::vector<std::unique_ptr<RegexRowMatcher>> regex_dfas;   // per batched query: the DFA-backed matcher of the rows handed back
        std::vector<std::unique_ptr<SubstringRowMatcher>> sub_matchers;   // ... and the substring matcher of the same
        std::vector<std::unique_ptr<RangeRowMatcher>> range_matchers;     // ... and the range matcher
        for (size_t i = 0; i < exprs.size(); ++i) {
            const RegexExpression *rx = i < regexes.size() ? regexes[i] : nullptr;
            const SubstringExpression *sx = subs && i < subs->size() ? (*subs)[i] : nullptr;
            const RangeExpression *rg = ranges && i < ranges->size() ? (*ranges)[i] : nullptr;
            // a range tree without DeviceMatch, or beside a regex or substring tree where the two families share no group: query()
            if (rg && (!cfg_.device_match || ((rx || sx) && !mix_ok))) {
                if (int32_t rc = query(exprs[i], results[i], rx, sx, rg, prefilter_of(i))) return rc;
                continue;
            }
            std::unique_ptr<SubstringRowMatcher> sub_matcher;
            if (sx && cfg_.device_match) {
                sub_matcher = std::make_unique<SubstringRowMatcher>(sx, cfg_.tokenizer);
                if (!sub_matcher->valid()) sub_matcher.reset();
            }
            std::unique_ptr<RegexRowMatcher> dfa;
            if (rx && cfg_.device_match && cfg_.device_regex) {
                dfa = std::make_unique<RegexRowMatcher>(rx, true);
                if (!dfa->valid()) dfa.reset();
            }
            if ((sx && !sub_matcher) || (rx && !dfa)) { if (int32_t rc = query(exprs[i], results[i], rx, sx, rg, prefilter_of(i))) return rc; continue; }
            live.push_back(i);
            live_regex.push_back(rx);
            live_sub.push_back(sx);
            live_range.push_back(rg);
            regex_dfas.push_back(std::move(dfa));
            sub_matchers.push_back(std::move(sub_matcher));
            range_matchers.push_back(rg ? std::make_unique<RangeRowMatcher>(rg) : nullptr);
        }
        if (live.empty()) return kEngineOk;
        const auto t_begin = std::chrono::steady_clock::now();
        std::vector<const BloomExpression *> batch, prune;
        std::vector<std::unique_ptr<BloomExpression>> prune_storage;
        for (size_t k = 0; k < live.size(); ++k) {
            batch.push_back(exprs[live[k]]);
            // pruneBloomQuery = AndBloomQueries(bloom, RegexFieldGuardBloomQuery(regex)), as query(); a plain query keeps its pointer
            if (!live_regex[k] && !live_sub[k] && !live_range[k]) { prune.push_back(batch[k]); continue; }
            BloomExpression guard, sub_guard, range_guard_storage, two, three;
            const bool has_guard = regex_field_guard(live_regex[k], guard);
            const bool has_two = and_bloom_queries(batch[k], has_guard ? &guard : nullptr, two);
            // ... the substring guard as its third side, the range guard as its fourth
            const bool has_sub_guard = substring_guard(live_sub[k], cfg_.tokenizer, sub_guard);
            const bool has_three = and_bloom_queries(has_two ? &two : nullptr, has_sub_guard ? &sub_guard : nullptr, three);
            const bool has_range_guard = range_guard(live_range[k], range_guard_storage);
            prune_storage.push_back(std::make_unique<BloomExpression>());
            prune.push_back(and_bloom_queries(has_three ? &three : nullptr, has_range_guard ? &range_guard_storage : nullptr, *prune_storage.back()) ? prune_storage.back().get() : nullptr);
        }
        std::vector<Survivors> sv;
        if (int32_t rc = probe_stage(prune, sv)) return rc;
        for (size_t k = 0; k < live.size(); ++k) apply_prefilter(prefilter_of(live[k]), sv[k]);
        const int64_t probe_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count();
        const auto t_scan = std::chrono::steady_clock::now();
        const size_t Q = live.size();
        std::vector<std::vector<ScanBlock>> scanned(Q);
        // per block (in file / block order): which queries scan it
        std::vector<std::vector<std::vector<uint8_t>>> wants(files_.size());
        for (size_t f = 0; f < files_.size(); ++f) wants[f].assign(files_[f].blocks.size(), std::vector<uint8_t>());
        for (size_t k = 0; k < Q; ++k) {
            size_t candidate_blocks = 0;
            for (size_t f = 0; f < files_.size(); ++f) if (sv[k].file_ok[f]) candidate_blocks += files_[f].blocks.size();
            const int64_t probe_share = candidate_blocks ? std::max<int64_t>(1, probe_ns / (int64_t)candidate_blocks) : 0;
            block_stage_stats(sv[k], probe_share, results[live[k]], scanned[k]);
            for (const ScanBlock &sb : scanned[k]) {
                if (wants[sb.f][sb.b].empty()) wants[sb.f][sb.b].assign(Q, 0);
                wants[sb.f][sb.b][k] = 1;
            }
        }
        std::vector<const std::string *> scan;
        std::vector<uint32_t> set_first{0};
        std::vector<const std::vector<uint8_t> *> set_wants;
        for (size_t f = 0; f < files_.size(); ++f)
            for (size_t b = 0; b < files_[f].blocks.size(); ++b) {
                if (wants[f][b].empty()) continue;
                for (const std::string &row : files_[f].blocks[b].rows) scan.push_back(&row);
                set_first.push_back((uint32_t)scan.size());
                set_wants.push_back(&wants[f][b]);
            }
        // hit[k][row]: only read where query k scans the row's set
        std::vector<std::vector<uint8_t>> hit(Q, std::vector<uint8_t>(scan.size(), 0));
        std::vector<RowMatcher> matchers;
        matchers.reserve(Q);
        for (size_t k = 0; k < Q; ++k) matchers.emplace_back(batch[k], cfg_.tokenizer);
        std::vector<uint8_t> on_device(Q, 0);
        // DeviceMatchHistogram: the queries with a histogram spec leave the batch's groups and form groups of their own per distinct spec
        std::vector<std::vector<uint64_t>> hist_counts(Q);
        std::vector<uint8_t> counted(Q, 0);                          // the device route decided query k's histogram
        if (cfg_.device_match && !scan.empty()) {
            std::vector<size_t> plain;
            std::map<HistSpec, std::vector<size_t>> by_spec;
            for (size_t k = 0; k < Q; ++k) {
                const HistSpec *hs = cfg_.device_match_histogram && hists && live[k] < hists->size() ? (*hists)[live[k]] : nullptr;
                if (hs) by_spec[*hs].push_back(k); else plain.push_back(k);
            }
            if (!plain.empty())
                if (int32_t rc = match_rows_device_many(batch, live_regex, live_sub, live_range, scan, set_first, set_wants, matchers, regex_dfas, sub_matchers, range_matchers, hit, on_device, plain)) return rc;
            for (const auto &kv : by_spec) {
                for (size_t k : kv.second) hist_counts[k].assign((size_t)kv.first.buckets + 3, 0);
                if (int32_t rc = match_rows_device_many(batch, live_regex, live_sub, live_range, scan, set_first, set_wants, matchers, regex_dfas, sub_matchers, range_matchers, hit, on_device, kv.second,
                                                        &kv.first, &hist_counts)) return rc;
                for (size_t k : kv.second) counted[k] = on_device[k];
            }
        }
        for (size_t k = 0; k < Q; ++k) {
            QueryResult &out = results[live[k]];
            if (counted[k]) {                                        // its rows were never listed: the counts are the answer
                out.hist = std::move(hist_counts[k]);
                add_scan_time(t_scan, scanned[k], out);
                continue;
            }
            // not decided in a group (alone beyond a limit, or the library refused the group): per query, as before.  query() probes
            // again and rewrites the stats block_stage_stats left here: known, and rare enough not to carry the survivors over
            if ((live_regex[k] || live_sub[k] || live_range[k]) && !on_device[k] && !scanned[k].empty()) {
                if (int32_t rc = query(exprs[live[k]], out, live_regex[k], live_sub[k], live_range[k], prefilter_of(live[k]))) return rc;
                continue;
            }
            for (size_t s = 0; s + 1 < set_first.size(); ++s) {
                if (!(*set_wants[s])[k]) continue;
                for (uint32_t i = set_first[s]; i < set_first[s + 1]; ++i) {
                    if (!on_device[k]) hit[k][i] = matchers[k].match(*scan[i]);
                    if (hit[k][i]) out.rows.push_back(*scan[i]);
                }
            }
            add_scan_time(t_scan, scanned[k], out);
        }
        return kEngineOk;
    }

private:
    // any of the keys under which query_many's groups take the wide or the lookup calls: range and text conditions share those only
    // under DeviceMatchRangeTextWide
    bool any_wide_key() const
    {
        return cfg_.device_match_wide || cfg_.device_match_wide_rows || cfg_.device_match_lookup || cfg_.device_match_lookup_rows;
    }
    void count_match_call(const char *entry_point)
    {
        std::lock_guard<std::mutex> lk(match_calls_mu_);
        ++match_calls_[entry_point];
    }
    mutable std::mutex match_calls_mu_;
    std::map<std::string, uint64_t> match_calls_;

    bsg_tokenizer c_tokenizer() const
    {
        bsg_tokenizer t{};
        t.sep_ascii[0] = cfg_.tokenizer.sep[0];
        t.sep_ascii[1] = cfg_.tokenizer.sep[1];
        t.flags = cfg_.tokenizer.flags | BSG_TOK_NGRAM(cfg_.tokenizer.ngram);
        return t;
    }

    struct PartitionBuffer {
        BloomEntrySets entries;
        std::vector<std::string> rows;
        uint64_t bytes = 0;
        std::vector<bsg_minmax> minmax;      // (host ingest route) one index per configured field, folded row by row
    };

    // ---- MinMax indexes ----
    // index[f] of the configured field f -> the block's map (absent indexes are left out, as the reference's map has no entry)
    void set_block_minmax(DataBlock &blk, const bsg_minmax *index, size_t n) const
    {
        blk.minmax.clear();
        for (size_t f = 0; f < n && f < cfg_.minmax_indexes.size(); ++f)
            if (index[f].present) blk.minmax[cfg_.minmax_indexes[f]] = bsg_minmax{index[f].min, index[f].max, 1, 0};
    }
    static bool same_minmax_keys(const DataBlock &a, const DataBlock &b)
    {
        if (a.minmax.size() != b.minmax.size()) return false;
        for (auto ia = a.minmax.begin(), ib = b.minmax.begin(); ia != a.minmax.end(); ++ia, ++ib)
            if (ia->first != ib->first) return false;
        return true;
    }
    // every row of every block on the host (a flush whose device route gave up on its tables)
    void host_minmax_blocks(DataFile &file) const
    {
        for (DataBlock &blk : file.blocks) {
            std::vector<bsg_minmax> index(cfg_.minmax_indexes.size(), bsg_minmax{});
            for (const std::string &r : blk.rows) minmax_row(r, cfg_.minmax_indexes, index.data());
            set_block_minmax(blk, index.data(), index.size());
        }
    }
    // the configured names packed like bsg_hash_entries' input
    void pack_minmax_fields(std::vector<uint8_t> &bytes, std::vector<uint32_t> &off) const
    {
        bytes.clear();
        off.assign(1, 0);
        for (const std::string &f : cfg_.minmax_indexes) { bytes.insert(bytes.end(), f.begin(), f.end()); off.push_back((uint32_t)bytes.size()); }
    }
    // A prefilter as a mask on what the probe stages left: a block failing the tree is neither scanned nor given a BlockStats entry
    // (block_ok 3), a file left without blocks counts in neither FilesConsidered nor FilesBloomSkipped (file_ok 2: the reference drops
    // it before the file stage, query_exec.go:390-396).
    template <class SurvivorsT>
    void apply_prefilter(const PrefilterExpression *pf, SurvivorsT &sv) const
    {
        if (!pf) return;
        for (size_t f = 0; f < files_.size(); ++f) {
            size_t kept = 0;
            for (size_t b = 0; b < files_[f].blocks.size(); ++b) {
                const DataBlock &blk = files_[f].blocks[b];
                if (prefilter_eval(*pf, PrefilterBlock{blk.partition_id, &blk.minmax})) ++kept;
                else sv.block_ok[f][b] = 3;
            }
            if (!kept) sv.file_ok[f] = 2;
        }
    }

    EngineConfig cfg_;
    bsg_ctx *ctx_;
    std::map<std::string, PartitionBuffer> buffers_;
    // DeviceIngestStream: the open streaming ingest of the rows in buffers_ (0 = none yet: opened by the first batch) and the set
    // every partition buffer got in it, numbered by first arrival (the blocks of a file are ordered by partition id)
    uint64_t stream_ = 0;
    std::map<std::string, uint32_t> stream_set_;
    std::vector<std::string> stream_keys_;   // DevicePartition: the text of every set of the keyed stream (bsg_ingest_keys), stream_set_ its inverse
    std::map<uint32_t, std::vector<bsg_minmax>> stream_minmax_host_;   // per set: the MinMax contributions of the rows the appends handed back
    bool stream_broken_ = false;         // an append failed (and ingest_rows said so): this flush builds from the kept rows
    StreamStats stream_stats_;
    uint64_t buffered_rows_ = 0, buffered_bytes_ = 0;
    std::vector<DataFile> files_;
    uint64_t next_file_id_ = 1;
    bool stopped_ = false;
    std::string err_;
    uint64_t files_arena_ = 0;           // the file-level filters of all files, one "block" per file
    bool files_arena_valid_ = false;
    std::vector<int32_t> file_status_;   // parseFilterSection outcome per file (0 ok)

    int32_t fail(int32_t code, std::string msg) { err_ = std::move(msg); return code; }

    // what the two probe stages leave of the files and blocks for one query: block_ok 0 pruned, 1 scanned, 2 unreadable filters
    struct Survivors {
        std::vector<uint8_t> file_ok;
        std::vector<std::vector<uint8_t>> block_ok;
    };
    struct ScanBlock { size_t f, b, stat; };        // a scanned block and its entry in block_stats

    // File stage and block stage for a batch of pruning expressions in ONE QueryBatch (a nil expression probes nothing: every
    // file and block stays).
    int32_t probe_stage(const std::vector<const BloomExpression *> &exprs, std::vector<Survivors> &sv)
    {
        sv.assign(exprs.size(), Survivors{});
        for (Survivors &s : sv) {
            s.file_ok.assign(files_.size(), 1);
            s.block_ok.resize(files_.size());
            for (size_t f = 0; f < files_.size(); ++f) s.block_ok[f].assign(files_[f].blocks.size(), 1);
        }
        QueryBatch qb;
        std::vector<size_t> probed;                 // batch query k = exprs[probed[k]]
        for (size_t i = 0; i < exprs.size(); ++i)
            if (exprs[i]) { qb.add_query(exprs[i]); probed.push_back(i); }
        if (probed.empty() || files_.empty()) return kEngineOk;
        const size_t Q = probed.size();
        std::vector<bsg_term> terms;
        if (int32_t rc = hash_terms(qb, terms)) return rc;
        uint64_t batch = 0;
        if (bsg_batch_create(ctx_, terms.data(), (uint32_t)terms.size(), qb.prog_ops.data(), qb.prog_off.data(), (uint32_t)Q, &batch))
            return fail(kErrGpu, bsg_last_error(ctx_));
        struct FreeBatch { bsg_ctx *c; uint64_t id; ~FreeBatch() { bsg_batch_free(c, id); } } guard{ctx_, batch};
        // file stage (query_exec.go:399-406): one probe over the file-level filters, one "block" per file
        if (int32_t rc = ensure_files_arena()) return rc;
        const size_t fw = (files_.size() + 63) / 64;
        std::vector<uint64_t> fs(Q * fw);
        if (bsg_probe_batch(ctx_, files_arena_, batch, 0, fs.data())) return fail(kErrGpu, bsg_last_error(ctx_));
        // block stage: only the files that passed (for any query), each through its arena - resident in the library's cache, or
        // decoded now and published there - all in one pipelined call; the leases end when the survivors are on the host
        std::vector<uint64_t> ids;
        std::vector<size_t> which;
        std::vector<FileLease> leases;
        struct ReleaseAll { bsg_ctx *c; std::vector<FileLease> &v; ~ReleaseAll() { for (auto &l : v) bsg_file_arena_release(c, l.lease); } } release{ctx_, leases};
        size_t words = 0;
        for (size_t f = 0; f < files_.size(); ++f) {
            bool any = false;
            for (size_t k = 0; k < Q; ++k) {
                // a corrupt file-level section decodes to nil filters: cannot disqualify
                any |= (sv[probed[k]].file_ok[f] = (fs[k * fw + (f >> 6)] >> (f & 63)) & 1) != 0;
            }
            if (!any || files_[f].blocks.empty()) continue;
            leases.emplace_back();
            if (int32_t rc = lease_file_arena(files_[f], leases.back())) { leases.pop_back(); return rc; }
            ids.push_back(leases.back().arena);
            which.push_back(f);
            words += Q * ((files_[f].blocks.size() + 63) / 64);
        }
        std::vector<uint64_t> bs(std::max<size_t>(words, 1));
        if (!ids.empty() && bsg_probe_many(ctx_, ids.data(), (uint32_t)ids.size(), batch, 0, bs.data()))
            return fail(kErrGpu, bsg_last_error(ctx_));
        size_t o = 0;
        for (size_t i = 0; i < which.size(); ++i) {
            const size_t f = which[i], bw = (files_[f].blocks.size() + 63) / 64;
            for (size_t k = 0; k < Q; ++k)
                for (size_t b = 0; b < files_[f].blocks.size(); ++b) {
                    const uint32_t r = leases[i].rows[b];                      // block b's row in the arena
                    uint8_t &ok = sv[probed[k]].block_ok[f][b];
                    ok = (bs[o + k * bw + (r >> 6)] >> (r & 63)) & 1;
                    if (leases[i].status[b] != 0) ok = 2;   // unreadable filters: neither pruned nor scanned (query_exec.go:580-590)
                }
            o += Q * bw;
        }
        return kEngineOk;
    }

    // One query's FilesConsidered / FilesBloomSkipped / BlockStats / Errors from what the probe stages left, and its scanned blocks.
    void block_stage_stats(const Survivors &sv, int64_t probe_share, QueryResult &out, std::vector<ScanBlock> &scanned)
    {
        for (size_t f = 0; f < files_.size(); ++f) {
            if (sv.file_ok[f] == 2) continue;                               // the prefilter left it no block: not considered at all
            out.files_considered++;
            if (!sv.file_ok[f]) { out.files_bloom_skipped++; continue; }   // file stage prune: no BlockStats for its blocks
            for (size_t b = 0; b < files_[f].blocks.size(); ++b) {
                if (sv.block_ok[f][b] == 3) continue;                       // failed the prefilter: neither scanned nor listed
                const DataBlock &blk = files_[f].blocks[b];
                BlockStats st;
                st.file_id = files_[f].file_id; st.block_offset = blk.block_offset;
                st.total_rows = (int64_t)blk.rows.size();
                st.total_bytes = (int64_t)(blk.row_bytes + blk.filter_section.size());
                st.duration_ns = probe_share;
                if (sv.block_ok[f][b] == 2) {        // recordUnreadBlocks (query_exec.go:625-639): totals only, error surfaced
                    out.errors.push_back("failed to read data block bloom filters: file " + std::to_string(files_[f].file_id) +
                                         " block offset " + std::to_string(blk.block_offset) + ": invalid hash");
                    out.block_stats.push_back(st);
                    continue;
                }
                if (!sv.block_ok[f][b]) {                                    // query_exec.go:607-614
                    st.bloom_filter_skipped = true;
                    out.block_stats.push_back(st);
                    continue;
                }
                for (const std::string &row : blk.rows) {
                    st.rows_processed++;
                    st.bytes_processed += (int64_t)row.size() + 4;
                }
                scanned.push_back(ScanBlock{f, b, out.block_stats.size()});
                out.block_stats.push_back(st);
            }
        }
    }

    void add_scan_time(std::chrono::steady_clock::time_point t_scan, const std::vector<ScanBlock> &scanned, QueryResult &out)
    {
        if (scanned.empty()) return;
        const int64_t scan_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_scan).count();
        for (const ScanBlock &sb : scanned) out.block_stats[sb.stat].duration_ns += std::max<int64_t>(1, scan_ns / (int64_t)scanned.size());
    }

    void drop_files_arena()
    {
        if (files_arena_valid_) bsg_arena_free(ctx_, files_arena_);
        files_arena_valid_ = false;
    }
    // ---- the file's block filters through the library's resident-arena cache (cache_api.inc) ----
    struct FileLease {
        uint64_t lease = 0, arena = 0;
        std::vector<uint32_t> rows;        // block b's row in the arena
        std::vector<int32_t> status;       // parseFilterSection outcome per block (0 ok); all 0 for a resident arena (only clean decodes stay)
    };
    static void file_key(const DataFile &f, uint8_t key[8]) { for (int i = 0; i < 8; ++i) key[i] = (uint8_t)(f.file_id >> (8 * i)); }
    // block keys (RowDataOffset) and the sections' extents in the (virtual) file's filter region
    static void block_extents(const DataFile &f, std::vector<uint64_t> &keys, std::vector<uint64_t> &begin, std::vector<uint64_t> &end)
    {
        uint64_t at = 0;
        for (auto &b : f.blocks) {
            keys.push_back(b.block_offset);
            begin.push_back(at);
            at += b.filter_section.size();
            end.push_back(at);
        }
    }
    void forget_file_arena(const DataFile &f)
    {
        uint8_t key[8];
        file_key(f, key);
        bsg_file_arena_forget(ctx_, key, 8);
    }
    void drop_arenas()
    {
        drop_files_arena();
        for (auto &f : files_) forget_file_arena(f);
    }
    // a freshly built / decoded arena of ALL the file's blocks becomes the cache's (and this lease's)
    int32_t publish_file_arena(const DataFile &f, uint64_t arena, const int32_t *status, FileLease &out)
    {
        uint8_t key[8];
        file_key(f, key);
        std::vector<uint64_t> keys, begin, end;
        block_extents(f, keys, begin, end);
        if (bsg_file_arena_publish(ctx_, key, 8, arena, keys.data(), begin.data(), end.data(), status, (uint32_t)keys.size(), &out.lease, nullptr)) {
            bsg_arena_free(ctx_, arena);
            return fail(kErrGpu, bsg_last_error(ctx_));
        }
        out.arena = arena;
        out.rows.resize(keys.size());
        for (size_t b = 0; b < keys.size(); ++b) out.rows[b] = (uint32_t)b;
        if (status) out.status.assign(status, status + keys.size()); else out.status.assign(keys.size(), 0);
        return kEngineOk;
    }
    int32_t lease_file_arena(const DataFile &f, FileLease &out)
    {
        uint8_t key[8];
        file_key(f, key);
        std::vector<uint64_t> keys;
        for (auto &b : f.blocks) keys.push_back(b.block_offset);
        out.rows.assign(keys.size(), 0);
        if (bsg_file_arena_acquire(ctx_, key, 8, keys.data(), (uint32_t)keys.size(), &out.lease, &out.arena, nullptr, out.rows.data()))
            return fail(kErrGpu, bsg_last_error(ctx_));
        if (out.lease) { out.status.assign(keys.size(), 0); return kEngineOk; }
        std::vector<const std::vector<uint8_t> *> bsec;
        for (auto &b : f.blocks) bsec.push_back(&b.filter_section);
        uint64_t arena = 0;
        std::vector<int32_t> status;
        if (int32_t rc = load_arena(bsec, arena, status)) return rc;
        return publish_file_arena(f, arena, status.data(), out);
    }

    // buildFilters for many entry-set triples at once: sizes via EstimateParameters(max(n,1), fpr),
    // one bsg_build, then encodeFilterSection per triple.
    int32_t build_sections(const std::vector<const BloomEntrySets *> &sets, std::vector<std::vector<uint8_t>> &sections)
    {
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets{0}, fstart{0};
        std::vector<bsg_filter_desc> desc(sets.size() * 3);
        uint64_t cursor = 0;
        for (size_t s = 0; s < sets.size(); ++s)
            for (uint32_t c = 0; c < 3; ++c) {
                const auto &set = sets[s]->set_of(c);
                uint64_t m = 0, k = 0;
                if (bsg_estimate_parameters(std::max<uint64_t>(set.size(), 1), cfg_.bloom_false_positive_rate, &m, &k))
                    return fail(kErrGpu, bsg_last_error(ctx_));
                desc[s * 3 + c] = bsg_filter_desc{cursor, m, (uint32_t)k, 0};
                cursor += ((m + 63) / 64 + 1) / 2 * 2;
                pack_entries(set, bytes, offsets);
                fstart.push_back((uint32_t)offsets.size() - 1);
            }
        // build + encodeFilterSection both on the device: only the section bytes cross PCIe
        uint64_t total = 0;
        if (bsg_sections_size(desc.data(), (uint32_t)sets.size(), &total)) return fail(kErrGpu, bsg_last_error(ctx_));
        std::vector<uint8_t> region(total);
        std::vector<uint64_t> sec_off(sets.size() + 1);
        if (bsg_build_sections(ctx_, bytes.data(), offsets.data(), (uint32_t)offsets.size() - 1, fstart.data(), desc.data(),
                               (uint32_t)desc.size(), std::max<uint64_t>(cursor, 2), region.data(), region.size(), sec_off.data()))
            return fail(kErrGpu, bsg_last_error(ctx_));
        split_sections(region, sec_off, sections);
        return kEngineOk;
    }

    static void split_sections(const std::vector<uint8_t> &region, const std::vector<uint64_t> &sec_off,
                               std::vector<std::vector<uint8_t>> &sections)
    {
        sections.resize(sec_off.size() - 1);
        for (size_t s = 0; s + 1 < sec_off.size(); ++s) sections[s].assign(region.begin() + sec_off[s], region.begin() + sec_off[s + 1]);
    }

    // the host walker's entry sets of the rows the device handed back -> bsg_ingest_add_entries (set index -> its entries)
    int32_t add_host_entries(uint64_t ing, const std::map<uint32_t, BloomEntrySets> &per_set)
    {
        std::vector<uint8_t> eb;
        std::vector<uint32_t> eo{0}, es, ek;
        for (auto &kv : per_set)
            for (uint32_t c = 0; c < 3; ++c) {
                const size_t before = eo.size() - 1;
                pack_entries(kv.second.set_of(c), eb, eo);
                es.insert(es.end(), eo.size() - 1 - before, kv.first);
                ek.insert(ek.end(), eo.size() - 1 - before, c);
            }
        if (bsg_ingest_add_entries(ctx_, ing, eb.data(), eo.data(), (uint32_t)es.size(), es.data(), ek.data()))
            return fail(kErrGpu, bsg_last_error(ctx_));
        return kEngineOk;
    }

    void drop_stream()
    {
        if (stream_) bsg_ingest_free(ctx_, stream_);
        stream_ = 0;
        stream_set_.clear();
        stream_keys_.clear();
        stream_minmax_host_.clear();
    }

    // DeviceIngestStream, ingest time (ingest.go:444-450 with indexRow on the device): one validated batch -> the open stream.
    // A partition id met for the first time gets the next set (bsg_ingest_add_sets, parent 0 = the file); the rows the device
    // walker hands back are walked here and now, while the batch is at hand.
    int32_t stream_append(const std::vector<std::string_view> &rows, const std::vector<std::string> &pids)
    {
        const bsg_tokenizer tok = c_tokenizer();
        const size_t nf = cfg_.minmax_indexes.size();
        if (!stream_ && nf) {                       // the appends fold the sets' MinMax indexes too
            std::vector<uint8_t> fb_bytes;
            std::vector<uint32_t> f_off;
            pack_minmax_fields(fb_bytes, f_off);
            if (bsg_ingest_open_minmax(ctx_, 0, nullptr, 1, nullptr, BSG_INGEST_TRUSTED_JSON, &tok, &stream_, fb_bytes.data(), f_off.data(), (uint32_t)nf))
                return fail(kErrGpu, bsg_last_error(ctx_));
        }
        if (!stream_ && bsg_ingest_open(ctx_, 0, nullptr, 1, nullptr, BSG_INGEST_TRUSTED_JSON /* ingest_rows validated every row */, &tok, &stream_))
            return fail(kErrGpu, bsg_last_error(ctx_));
        std::vector<uint32_t> set_of_row(rows.size());
        uint32_t n_new = 0;
        for (size_t i = 0; i < rows.size(); ++i) {
            auto it = stream_set_.find(pids[i]);
            if (it == stream_set_.end()) { it = stream_set_.emplace(pids[i], (uint32_t)stream_set_.size()).first; ++n_new; }
            set_of_row[i] = it->second;
        }
        if (n_new) {
            const std::vector<uint32_t> parent(n_new, 0);
            uint32_t first = 0;
            if (bsg_ingest_add_sets(ctx_, stream_, n_new, parent.data(), nullptr, &first)) return fail(kErrGpu, bsg_last_error(ctx_));
        }
        std::vector<uint8_t> bytes;                 // this batch only: the rows of a batch are not contiguous in the caller's buffer
        std::vector<uint64_t> row_off{0};
        for (std::string_view r : rows) { bytes.insert(bytes.end(), r.begin(), r.end()); row_off.push_back(bytes.size()); }
        std::vector<uint32_t> fb(rows.size());
        uint32_t n_fb = 0;
        if (bsg_ingest_append_rows(ctx_, stream_, bytes.data(), row_off.data(), (uint32_t)rows.size(), set_of_row.data(), fb.data(),
                                   (uint32_t)fb.size(), &n_fb))
            return fail(kErrGpu, bsg_last_error(ctx_));
        if (n_fb) {
            std::map<uint32_t, BloomEntrySets> per_set;
            for (uint32_t i = 0; i < n_fb; ++i) {
                per_set.try_emplace(set_of_row[fb[i]], cfg_.tokenizer).first->second.index_row(rows[fb[i]]);
                if (nf) {                           // ... and folded on the host: the device decided nothing of such a row, or the same values
                    std::vector<bsg_minmax> &idx = stream_minmax_host_[set_of_row[fb[i]]];
                    idx.resize(nf, bsg_minmax{});
                    minmax_row(rows[fb[i]], cfg_.minmax_indexes, idx.data());
                }
            }
            if (int32_t rc = add_host_entries(stream_, per_set)) return rc;
        }
        stream_stats_.batches += 1;
        stream_stats_.rows += rows.size();
        stream_stats_.host_rows += n_fb;
        return kEngineOk;
    }

    // DevicePartition: the texts of the sets the keyed stream has made since the last look (bsg_ingest_keys) join stream_keys_ / stream_set_
    int32_t stream_fetch_keys()
    {
        uint32_t n = 0;
        uint64_t n_bytes = 0;
        const uint32_t first = (uint32_t)stream_keys_.size();
        if (bsg_ingest_keys(ctx_, stream_, first, nullptr, 0, nullptr, &n, &n_bytes)) return fail(kErrGpu, bsg_last_error(ctx_));
        if (!n) return kEngineOk;
        std::vector<uint8_t> kb((size_t)n_bytes + 1);
        std::vector<uint32_t> ko((size_t)n + 1);
        if (bsg_ingest_keys(ctx_, stream_, first, kb.data(), n_bytes, ko.data(), &n, &n_bytes)) return fail(kErrGpu, bsg_last_error(ctx_));
        for (uint32_t i = 0; i < n; ++i) {
            stream_keys_.emplace_back(reinterpret_cast<const char *>(kb.data()) + ko[i], ko[i + 1] - ko[i]);
            stream_set_.emplace(stream_keys_.back(), first + i);
        }
        return kEngineOk;
    }

    // DevicePartition, ingest time: stream_append with the partition ids found by the device.  pids[i] is filled from the texts of the
    // stream's sets; a row the partitioner hands back is parsed here (validate_object_row, the only rows it runs over), its text
    // registered (bsg_ingest_add_sets_keyed), and the row finished by the host walker with the other fallback rows.
    int32_t stream_append_keyed(const std::vector<std::string_view> &rows, std::vector<std::string> &pids)
    {
        const bsg_tokenizer tok = c_tokenizer();
        const size_t nf = cfg_.minmax_indexes.size();
        if (!stream_) {
            std::vector<uint8_t> fb_bytes;
            std::vector<uint32_t> f_off;
            if (nf) pack_minmax_fields(fb_bytes, f_off);
            if (bsg_ingest_open_keyed(ctx_, 1, 0, BSG_INGEST_TRUSTED_JSON /* TrustedRows */, &tok, &stream_,
                                      reinterpret_cast<const uint8_t *>(cfg_.partition_field.data()), (uint32_t)cfg_.partition_field.size(),
                                      nf ? fb_bytes.data() : nullptr, nf ? f_off.data() : nullptr, (uint32_t)nf))
                return fail(kErrGpu, bsg_last_error(ctx_));
        }
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> row_off{0};
        for (std::string_view r : rows) { bytes.insert(bytes.end(), r.begin(), r.end()); row_off.push_back(bytes.size()); }
        std::vector<uint32_t> set_of_row(rows.size()), fb(rows.size());
        uint32_t n_fb = 0, n_new = 0;
        if (bsg_ingest_append_rows_keyed(ctx_, stream_, bytes.data(), row_off.data(), (uint32_t)rows.size(), set_of_row.data(), &n_new, fb.data(),
                                         (uint32_t)fb.size(), &n_fb))
            return fail(kErrGpu, bsg_last_error(ctx_));
        if (n_new) if (int32_t rc = stream_fetch_keys()) return rc;
        // the rows the partitioner did not decide: their texts from the host parse, new ones registered in row order
        std::vector<uint32_t> undecided;
        std::vector<std::string> texts;
        std::string scratch;
        for (uint32_t i = 0; i < n_fb; ++i) {
            if (set_of_row[fb[i]] != BSG_SET_UNDECIDED) continue;
            std::string text;
            bool has = false;
            if (!validate_object_row(rows[fb[i]], cfg_.partition_field, text, has, scratch))
                return fail(kErrInvalidRow, "row " + std::to_string(fb[i]) + " is not a JSON object");
            if (!has) text.clear();
            undecided.push_back(fb[i]);
            texts.push_back(std::move(text));
        }
        if (!undecided.empty()) {
            std::vector<uint8_t> kb;
            std::vector<uint32_t> ko{0}, sets(texts.size());
            for (const std::string &t : texts) { kb.insert(kb.end(), t.begin(), t.end()); ko.push_back((uint32_t)kb.size()); }
            kb.push_back(0);
            if (bsg_ingest_add_sets_keyed(ctx_, stream_, kb.data(), ko.data(), (uint32_t)texts.size(), sets.data())) return fail(kErrGpu, bsg_last_error(ctx_));
            if (int32_t rc = stream_fetch_keys()) return rc;
            for (size_t i = 0; i < undecided.size(); ++i) set_of_row[undecided[i]] = sets[i];
        }
        for (size_t i = 0; i < rows.size(); ++i) {
            if (set_of_row[i] >= stream_keys_.size()) return fail(kErrGpu, "the keyed ingest named a set without a text");
            pids[i] = stream_keys_[set_of_row[i]];
        }
        if (n_fb) {
            std::map<uint32_t, BloomEntrySets> per_set;
            for (uint32_t i = 0; i < n_fb; ++i) {
                per_set.try_emplace(set_of_row[fb[i]], cfg_.tokenizer).first->second.index_row(rows[fb[i]]);
                if (nf) {
                    std::vector<bsg_minmax> &idx = stream_minmax_host_[set_of_row[fb[i]]];
                    idx.resize(nf, bsg_minmax{});
                    minmax_row(rows[fb[i]], cfg_.minmax_indexes, idx.data());
                }
            }
            if (int32_t rc = add_host_entries(stream_, per_set)) return rc;
        }
        stream_stats_.batches += 1;
        stream_stats_.rows += rows.size();
        stream_stats_.host_rows += n_fb;
        return kEngineOk;
    }

    // DeviceIngestStream, flush time: what is left of build_sections_device once every batch has been walked — finish, size,
    // bsg_ingest_build_sections.  The stream numbers its sets by first arrival, the file orders its blocks by partition id: the
    // sections and counts are permuted into block order, and no resident arena is asked for (its block i would be set i); the
    // file's arena is decoded from the stored sections by the first query, as without DeviceIngest.
    int32_t build_sections_stream(DataFile &file, std::vector<std::vector<uint8_t>> &sections, bool &minmax_done)
    {
        const size_t nb = file.blocks.size();
        std::vector<uint32_t> set_of_block(nb);
        for (size_t b = 0; b < nb; ++b) {
            auto it = stream_set_.find(file.blocks[b].partition_id);
            if (it == stream_set_.end() || stream_set_.size() != nb)    // every buffered row was appended: anything else is a bug here
                return fail(kErrGpu, "the streaming ingest does not hold the partitions of this flush");
            set_of_block[b] = it->second;
        }
        if (const size_t nf = cfg_.minmax_indexes.size()) {    // what the appends folded on the device, and the handed-back rows' share
            std::vector<bsg_minmax> index(nb * nf);
            if (bsg_ingest_minmax(ctx_, stream_, index.data(), index.size())) return fail(kErrGpu, bsg_last_error(ctx_));
            for (size_t b = 0; b < nb; ++b) {
                bsg_minmax *idx = index.data() + (size_t)set_of_block[b] * nf;
                const auto host = stream_minmax_host_.find(set_of_block[b]);
                for (size_t f = 0; f < nf && host != stream_minmax_host_.end(); ++f)
                    if (host->second[f].present) minmax_fold(idx[f], host->second[f].min, host->second[f].max);
                set_block_minmax(file.blocks[b], idx, nf);
            }
            minmax_done = true;
        }
        std::vector<uint64_t> counts((nb + 1) * 3);
        std::vector<uint32_t> status(nb + 1);
        if (bsg_ingest_finish(ctx_, stream_, counts.data(), status.data())) return fail(kErrGpu, bsg_last_error(ctx_));
        for (uint32_t st : status)
            if (st != 0) return build_sections_host_rows(file, sections);   // a set the device tables cannot represent (2^-62/entry)
        std::vector<bsg_filter_desc> desc((nb + 1) * 3);
        for (size_t i = 0; i < desc.size(); ++i) {
            uint64_t m = 0, k = 0;
            if (bsg_estimate_parameters(std::max<uint64_t>(counts[i], 1), cfg_.bloom_false_positive_rate, &m, &k))
                return fail(kErrGpu, bsg_last_error(ctx_));
            desc[i] = bsg_filter_desc{0, m, (uint32_t)k, 0};    // (word_off: the sections route lays the words out itself)
        }
        uint64_t total = 0;
        if (bsg_sections_size(desc.data(), (uint32_t)nb + 1, &total)) return fail(kErrGpu, bsg_last_error(ctx_));
        std::vector<uint8_t> region(total);
        std::vector<uint64_t> sec_off(nb + 2);
        if (bsg_ingest_build_sections(ctx_, stream_, desc.data(), region.data(), region.size(), sec_off.data(), nullptr, nullptr))
            return fail(kErrGpu, bsg_last_error(ctx_));
        std::vector<std::vector<uint8_t>> by_set;
        split_sections(region, sec_off, by_set);
        sections.resize(nb + 1);
        for (size_t b = 0; b <= nb; ++b) {
            const size_t s = b < nb ? set_of_block[b] : nb;
            sections[b] = std::move(by_set[s]);
            BloomEntryCounts &bc = b < nb ? file.blocks[b].counts : file.counts;
            bc = BloomEntryCounts{counts[s * 3], counts[s * 3 + 1], counts[s * 3 + 2]};
        }
        return kEngineOk;
    }

    // Device ingest of one file's blocks (flush.go:179-254 / merge.go:706-804 with a1-a5 on the GPU): rows ->
    // bsg_ingest_rows, the rows it hands back -> host walker -> bsg_ingest_add_entries, exact counts ->
    // EstimateParameters on the host -> bsg_ingest_build -> encodeFilterSection.  Fills the blocks' and the
    // file's BloomEntryCounts.  sections = one per block, then the file-level one.
    // minmax_done (flush only; merge unions its sources' indexes): the call computes the blocks' MinMax indexes too
    // (bsg_ingest_rows_minmax), the rows it hands back folded on the host in the loop that walks them; set to true once they are in.
    int32_t build_sections_device(DataFile &file, std::vector<std::vector<uint8_t>> &sections, bool *minmax_done = nullptr)
    {
        const size_t nb = file.blocks.size();
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> row_off{0};
        std::vector<uint32_t> first{0}, parent(nb, 0), set_of_row;
        for (size_t b = 0; b < nb; ++b) {
            for (const std::string &r : file.blocks[b].rows) {
                bytes.insert(bytes.end(), r.begin(), r.end());
                row_off.push_back(bytes.size());
                set_of_row.push_back((uint32_t)b);
            }
            first.push_back((uint32_t)set_of_row.size());
        }
        uint64_t ing = 0;
        const bsg_tokenizer tok = c_tokenizer();
        const size_t nf = minmax_done && !*minmax_done ? cfg_.minmax_indexes.size() : 0;
        if (nf) {
            std::vector<uint8_t> f_bytes;
            std::vector<uint32_t> f_off;
            pack_minmax_fields(f_bytes, f_off);
            if (bsg_ingest_rows_minmax(ctx_, bytes.data(), row_off.data(), (uint32_t)set_of_row.size(), first.data(), (uint32_t)nb, parent.data(), 1, nullptr,
                                       BSG_INGEST_TRUSTED_JSON, &tok, &ing, f_bytes.data(), f_off.data(), (uint32_t)nf))
                return fail(kErrGpu, bsg_last_error(ctx_));
        } else if (bsg_ingest_rows_tok(ctx_, bytes.data(), row_off.data(), (uint32_t)set_of_row.size(), first.data(), (uint32_t)nb,
                                       parent.data(), 1, nullptr, BSG_INGEST_TRUSTED_JSON /* ingest_rows validated every row */, &tok, &ing))
            return fail(kErrGpu, bsg_last_error(ctx_));
        struct Free { bsg_ctx *c; uint64_t id; ~Free() { bsg_ingest_free(c, id); } } guard{ctx_, ing};
        std::vector<bsg_minmax> index(nb * nf);
        if (nf && bsg_ingest_minmax(ctx_, ing, index.data(), index.size())) return fail(kErrGpu, bsg_last_error(ctx_));
        uint32_t n_fb = 0;
        if (bsg_ingest_fallback_rows(ctx_, ing, nullptr, 0, &n_fb)) return fail(kErrGpu, bsg_last_error(ctx_));
        if (n_fb) {
            std::vector<uint32_t> fb(n_fb);
            if (bsg_ingest_fallback_rows(ctx_, ing, fb.data(), n_fb, &n_fb)) return fail(kErrGpu, bsg_last_error(ctx_));
            std::map<uint32_t, BloomEntrySets> per_set;
            for (uint32_t r : fb) {
                const uint32_t b = set_of_row[r];
                per_set.try_emplace(b, cfg_.tokenizer).first->second.index_row(file.blocks[b].rows[r - first[b]]);
                if (nf) minmax_row(file.blocks[b].rows[r - first[b]], cfg_.minmax_indexes, index.data() + (size_t)b * nf);
            }
            if (int32_t rc = add_host_entries(ing, per_set)) return rc;
        }
        if (nf) {
            for (size_t b = 0; b < nb; ++b) set_block_minmax(file.blocks[b], index.data() + b * nf, nf);
            *minmax_done = true;
        }
        std::vector<uint64_t> counts((nb + 1) * 3);
        std::vector<uint32_t> status(nb + 1);
        if (bsg_ingest_finish(ctx_, ing, counts.data(), status.data())) return fail(kErrGpu, bsg_last_error(ctx_));
        for (uint32_t st : status)
            if (st != 0) return build_sections_host_rows(file, sections);   // a set the device tables cannot represent (2^-62/entry)
        std::vector<bsg_filter_desc> desc((nb + 1) * 3);
        uint64_t cursor = 0;
        for (size_t i = 0; i < desc.size(); ++i) {
            uint64_t m = 0, k = 0;
            if (bsg_estimate_parameters(std::max<uint64_t>(counts[i], 1), cfg_.bloom_false_positive_rate, &m, &k))
                return fail(kErrGpu, bsg_last_error(ctx_));
            desc[i] = bsg_filter_desc{cursor, m, (uint32_t)k, 0};
            cursor += ((m + 63) / 64 + 1) / 2 * 2;
        }
        uint64_t total = 0;
        if (bsg_sections_size(desc.data(), (uint32_t)nb + 1, &total)) return fail(kErrGpu, bsg_last_error(ctx_));
        std::vector<uint8_t> region(total);
        std::vector<uint64_t> sec_off(nb + 2);
        // the block filters stay on the device as this file's probe arena: a query right after the flush uploads nothing
        forget_file_arena(file);
        uint64_t built_arena = 0;
        if (bsg_ingest_build_sections(ctx_, ing, desc.data(), region.data(), region.size(), sec_off.data(), &built_arena, nullptr))
            return fail(kErrGpu, bsg_last_error(ctx_));
        split_sections(region, sec_off, sections);
        uint64_t blk_off = 0;
        for (size_t s = 0; s < nb; ++s) {        // what the cache records: the blocks' keys (RowDataOffset, as the callers assign it) and section extents
            file.blocks[s].filter_section = sections[s];
            file.blocks[s].block_offset = blk_off;
            blk_off += file.blocks[s].row_bytes;
        }
        if (built_arena) {                       // 0: the context does not keep this arena; decoded from the sections on first use
            FileLease l;
            if (int32_t rc = publish_file_arena(file, built_arena, nullptr, l)) return rc;
            bsg_file_arena_release(ctx_, l.lease);
        }
        for (size_t s = 0; s <= nb; ++s) {
            BloomEntryCounts &bc = s < nb ? file.blocks[s].counts : file.counts;
            bc = BloomEntryCounts{counts[s * 3], counts[s * 3 + 1], counts[s * 3 + 2]};
        }
        return kEngineOk;
    }

    // Host walker over every row of the file (the reference's own order of work), filters still built on the GPU.
    int32_t build_sections_host_rows(DataFile &file, std::vector<std::vector<uint8_t>> &sections)
    {
        std::vector<std::unique_ptr<BloomEntrySets>> block_sets;
        BloomEntrySets file_entries;
        std::vector<const BloomEntrySets *> sets;
        for (auto &blk : file.blocks) {
            block_sets.push_back(std::make_unique<BloomEntrySets>(cfg_.tokenizer));
            for (const std::string &r : blk.rows) block_sets.back()->index_row(r);
            blk.counts = block_sets.back()->counts();
            block_sets.back()->union_into(file_entries);
            sets.push_back(block_sets.back().get());
        }
        sets.push_back(&file_entries);
        file.counts = file_entries.counts();
        return build_sections(sets, sections);
    }

    // matchRowBytes for the whole scan list in one bsg_match_rows call.  on_device stays false (and the host matcher
    // takes over) when the expression is beyond the device matcher's limits.
    // compileRowMatcher's root And(bloom root, regex root) (row_matcher.go:353-368) as one bsg_match_rows_regex program; the regex
    // side lowered by compileRegexExpression's rules (row_matcher.go:440-480).  on_device stays false when the library answers
    // BSG_E_UNSUPPORTED (too many conditions, tables over its LDS cap): the caller takes the host path.
    static void lower_regex(const RegexExpression &e, MatcherProgram &mp)
    {
        switch (e.type) {
        case RegexType::Condition:
            if (!e.has_condition) { mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0)); return; }
            if (e.field.empty()) { mp.prog_ops.push_back(BSG_OP(BSG_OP_FALSE, 0)); return; }
            mp.prog_ops.push_back(BSG_OP(BSG_OP_TERM, (uint32_t)mp.kinds.size()));
            mp.kinds.push_back(BSG_KIND_FIELD_REGEX);
            mp.fields.push_back(e.field);
            mp.tokens.push_back(e.pattern);
            return;
        case RegexType::And:
        case RegexType::Or:
            if (e.children.empty()) { mp.prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_TRUE : BSG_OP_FALSE, 0)); return; }
            for (auto &c : e.children) lower_regex(c, mp);
            mp.prog_ops.push_back(BSG_OP(e.type == RegexType::And ? BSG_OP_AND : BSG_OP_OR, (uint32_t)e.children.size()));
            return;
        default:
            mp.prog_ops.push_back(BSG_OP(BSG_OP_FALSE, 0));
        }
    }
    int32_t match_rows_device_regex(const BloomExpression *expr, const RegexExpression &regex, const std::vector<const std::string *> &scan,
                                    RowMatcher &host_matcher, RegexRowMatcher &host_regex, std::vector<uint8_t> &hit, bool &on_device)
    {
        MatcherProgram mp(expr);
        if (!expr) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        lower_regex(regex, mp);
        mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 2));
        std::vector<uint8_t> cbytes;
        std::vector<uint32_t> coff{0};
        for (size_t c = 0; c < mp.kinds.size(); ++c) {
            cbytes.insert(cbytes.end(), mp.fields[c].begin(), mp.fields[c].end()); coff.push_back((uint32_t)cbytes.size());
            cbytes.insert(cbytes.end(), mp.tokens[c].begin(), mp.tokens[c].end()); coff.push_back((uint32_t)cbytes.size());
        }
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> row_off{0};
        for (const std::string *r : scan) { bytes.insert(bytes.end(), r->begin(), r->end()); row_off.push_back(bytes.size()); }
        std::vector<uint64_t> bits((scan.size() + 63) / 64);
        std::vector<uint32_t> fb(scan.size());
        uint32_t n_fb = 0;
        const bsg_tokenizer tok = c_tokenizer();
        count_match_call("bsg_match_rows_tok");
        const int32_t rc = bsg_match_rows_tok(ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(),
                                              mp.kinds.data(), (uint32_t)mp.kinds.size(), mp.prog_ops.data(), (uint32_t)mp.prog_ops.size(), &tok,
                                              bits.data(), fb.data(), (uint32_t)fb.size(), &n_fb);
        if (rc == BSG_E_UNSUPPORTED) return kEngineOk;
        if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
        for (size_t i = 0; i < scan.size(); ++i) hit[i] = (bits[i >> 6] >> (i & 63)) & 1;
        for (uint32_t i = 0; i < n_fb; ++i) {
            const std::string &row = *scan[fb[i]];
            hit[fb[i]] = host_matcher.match(row) && host_regex.match(row);
        }
        on_device = true;
        return kEngineOk;
    }

    // The scan list under DeviceMatch for a batch: queries are packed, in order, into groups of <= 64 queries over <= 64 distinct
    // conditions (deduplicated across the group's queries by (kind, field, token or pattern)); one call per group with the sets'
    // masks restricted to the group: bsg_match_rows_many_regex for a group with a regex condition, bsg_match_rows_many otherwise.
    // A regex query's program is And(bloom root | TRUE, regex root).  A group also closes when the next query would bring it over 16
    // regex conditions, over the batched kernel's table bytes (by regex_groups.hpp's estimate) or would let one leaf lie under
    // more regex conditions than a lane holds (co_active_bound).  on_device[k] stays 0 (the caller decides query k by itself) for
    // a query beyond one of these limits alone or a group the library answers BSG_E_UNSUPPORTED for.
    // Under DeviceMatchLookup(Rows) a group without a regex condition is bounded by 1 024 conditions and decided by bsg_match_rows_lookup(_rows);
    // with DeviceMatchLookupRegex one WITH regex conditions is too, decided by bsg_match_rows_lookup_regex(_rows), its regex tables
    // bounded by bsh_lookup::rx_lds_cap_of over the group's table (strings <= 2 x its other conditions, pairs <= its FieldToken ones).
    // Under DeviceMatchWide a group has no member limit (and the storing walker's larger table cap): one bsg_match_rows_wide call per
    // group, each set's CSR query list read from set_wants; its result holds a bit row per (set, listed query) only.
    // A query with a substring tree (subs[k]) adds And(.., substring root) to its program and its Substring / FieldSubstring conditions
    // to the table.  A group with a needle also closes where the next query's needles would no longer pack beside its own, and its
    // regex tables are bounded by the reduced cap beside a needle table (substring_groups.hpp fits); it is decided by
    // bsg_match_rows_many_substr / bsg_match_rows_many_regex_substr, under the wide keys by bsg_match_rows_wide_substr(_rows), and never by
    // a lookup call (under the lookup keys it takes the wide route, bounded by 64 conditions).
    // A query with a range tree (ranges[k]; it has neither of the other two) is And(bloom root | TRUE, range root) with its FieldRange
    // conditions in the table.  A group closes where the next query would put a range condition beside a regex or substring one, in either
    // order (range_groups.hpp joins); plain queries go with both.  A group with a range condition is decided by bsg_match_rows_many_range,
    // under the wide keys by bsg_match_rows_wide_range(_rows), and never by a lookup call (the wide route, bounded by 64 conditions).
    // Under DeviceMatchRangeTextWide (with DeviceMatchRangeText and a wide or lookup key) range and text conditions share a wide group: it
    // closes by range_text_groups.hpp's wide rules (the regex tables under 42 496 bytes needle or not), is decided by ONE
    // bsg_match_rows_wide_regex_substr_range(_rows) call, and is a 64-condition wide group under the lookup keys, never a lookup call's.
    int32_t match_rows_device_many(const std::vector<const BloomExpression *> &exprs, const std::vector<const RegexExpression *> &regexes,
                                   const std::vector<const SubstringExpression *> &subs, const std::vector<const RangeExpression *> &ranges,
                                   const std::vector<const std::string *> &scan, const std::vector<uint32_t> &set_first,
                                   const std::vector<const std::vector<uint8_t> *> &set_wants, std::vector<RowMatcher> &host_matchers,
                                   std::vector<std::unique_ptr<RegexRowMatcher>> &host_regex, std::vector<std::unique_ptr<SubstringRowMatcher>> &host_sub,
                                   std::vector<std::unique_ptr<RangeRowMatcher>> &host_range,
                                   std::vector<std::vector<uint8_t>> &hit, std::vector<uint8_t> &on_device, const std::vector<size_t> &order,
                                   const HistSpec *hist = nullptr, std::vector<std::vector<uint64_t>> *hist_counts = nullptr)
    {
        // order: the queries this pass groups, ascending.  hist (under a wide key): every group is decided by ONE bsg_match_rows_wide_hist
        // call with this spec, and (*hist_counts)[k] takes query k's buckets + 3 counts summed over its sets; hit is not written
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> row_off{0};
        for (const std::string *r : scan) { bytes.insert(bytes.end(), r->begin(), r->end()); row_off.push_back(bytes.size()); }
        const bsg_tokenizer tok = c_tokenizer();
        const size_t n_words = (scan.size() + 63) / 64, n_sets = set_wants.size();
        // DeviceMatchWide: a group is bounded by its table, not by its members; the storing walker's LDS leaves the tables more room
        // DeviceMatchLookup: the wide call's groups; one without a regex condition may hold 1 024 conditions and takes the lookup call
        const bool lookup_rows = !hist && cfg_.device_match_lookup_rows, lookup = !hist && (cfg_.device_match_lookup || lookup_rows);   // (the hist call is a wide call: 64 conditions)
        const bool wide_rows = cfg_.device_match_wide_rows || lookup_rows, wide = cfg_.device_match_wide || wide_rows || lookup;
        const bool lookup_regex = lookup && cfg_.device_match_lookup_regex;
        // range and text conditions may share a group: without a wide key by DeviceMatchRangeText, under one by DeviceMatchRangeTextWide as well
        const bool wide_mix = bsh_rtg::wide_mixing(cfg_.device_match, cfg_.device_match_range_text, cfg_.device_match_range_text_wide, wide);
        const bool mix_ok = bsh_rtg::mixing(cfg_.device_match, cfg_.device_match_range_text, wide) || wide_mix;
        const size_t max_members = wide ? bsh_wide::kMaxQueries : 64;
        const uint32_t table_cap = wide ? bsh_wide::kWideLdsCap : bsh_rxg::kManyLdsCap;
        std::map<std::string, std::pair<uint32_t, uint32_t>> dfa_size;      // pattern -> (states, classes); (0, 0): outside the subset
        auto rx_bytes = [&](const std::string &field, const std::string &pattern) -> uint32_t {
            auto it = dfa_size.find(pattern);
            if (it == dfa_size.end()) {
                bsh_rx::Dfa d;
                std::string err;
                const bool ok = bsh_rx::compile(pattern, d, err);
                it = dfa_size.emplace(pattern, ok ? std::make_pair(d.n_states, d.n_classes) : std::make_pair(0u, 0u)).first;
            }
            return bsh_rxg::rx_table_bytes(it->second.first, it->second.second, (uint32_t)field.size(), !wide);   // the wide blob holds no user masks
        };
        size_t pos = 0;
        while (pos < order.size()) {
            // the group's table and programs
            std::map<std::tuple<uint32_t, std::string, std::string>, uint32_t> index;
            std::vector<uint32_t> kinds, prog_ops, prog_off{0};
            std::vector<std::string> fields, tokens;
            std::vector<size_t> members;
            uint32_t n_rx = 0, rx_table = 0;                                 // the group's regex conditions and their table bytes
            uint32_t n_plain = 0, n_ft = 0;                                  // its other conditions, and the FieldToken ones among them
            bsh_subg::Group sub_group;                                       // its needles as they pack, and rx_table once more
            bsh_rngg::Mix mix;                                               // whether its table holds a range / a regex or substring condition
            for (; pos < order.size() && members.size() < max_members; ++pos) {
                const size_t k = order[pos];
                MatcherProgram mp(exprs[k]);
                if (regexes[k] || subs[k] || ranges[k]) {   // And(bloom root | TRUE, the trees the query has); a range tree beside the others only under mix_ok
                    if (!exprs[k] || mp.prog_ops.empty()) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
                    if (regexes[k]) lower_regex(*regexes[k], mp);
                    if (subs[k]) emit_substring_program(*subs[k], mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
                    if (ranges[k]) emit_range_program(*ranges[k], mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
                    mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 1u + (regexes[k] ? 1u : 0u) + (subs[k] ? 1u : 0u) + (ranges[k] ? 1u : 0u)));
                }
                // what the query adds: distinct conditions, regex conditions, table bytes, and the fields that may meet on a leaf
                std::map<std::tuple<uint32_t, std::string, std::string>, uint32_t> added;
                uint32_t fresh_rx = 0, fresh_bytes = 0, fresh_plain = 0, fresh_ft = 0;
                bsh_subg::Fresh fresh_sub;                                   // the folded lengths of its fresh needles, in condition order
                bsh_rngg::Mix query_mix;
                for (size_t c = 0; c < mp.kinds.size(); ++c) query_mix.see(mp.kinds[c]);
                for (size_t c = 0; c < mp.kinds.size(); ++c) {
                    const auto key = std::make_tuple(mp.kinds[c], mp.fields[c], mp.tokens[c]);
                    if (index.count(key) || !added.emplace(key, 0).second) continue;
                    if (mp.kinds[c] == BSG_KIND_FIELD_REGEX) { ++fresh_rx; fresh_bytes += rx_bytes(mp.fields[c], mp.tokens[c]); }
                    else if (mp.kinds[c] == BSG_KIND_SUBSTRING || mp.kinds[c] == BSG_KIND_FIELD_SUBSTRING) {
                        std::string folded;
                        (void)fold_needle(mp.tokens[c], cfg_.tokenizer, folded);       // valid: the caller kept the query in the batch
                        fresh_sub.needle_len.push_back((uint32_t)folded.size());
                    }
                    else { ++fresh_plain; fresh_ft += mp.kinds[c] == BSG_KIND_FIELD_TOKEN ? 1u : 0u; }
                }
                fresh_sub.rx_bytes = fresh_bytes;
                std::vector<std::string_view> rx_fields;
                for (size_t c = 0; c < kinds.size(); ++c) if (kinds[c] == BSG_KIND_FIELD_REGEX) rx_fields.push_back(fields[c]);
                for (const auto &kv : added) if (std::get<0>(kv.first) == BSG_KIND_FIELD_REGEX) rx_fields.push_back(std::get<1>(kv.first));
                const bool rx_group = n_rx + fresh_rx != 0;
                const bool needle_group = sub_group.n_needles + fresh_sub.needle_len.size() != 0;   // never a lookup call's
                const bool range_group = mix.range || query_mix.range;                              // nor is this one
                const size_t cond_cap = bsh_rngg::lookup_group(lookup, lookup_regex, range_group, rx_group, needle_group) ? bsh_lookup::kMaxConds : 64;
                // the lookup regex call's cap depends on the table: what this group's strings and pairs can take at most
                const uint32_t group_cap = lookup_regex && rx_group && !needle_group ? bsh_lookup::rx_lds_cap_of(2u * (n_plain + fresh_plain), n_ft + fresh_ft) : table_cap;
                // a table with kind 6 beside a text condition: the reduced cap beside a needle table, needle or not (range_text_groups.hpp)
                // ... and in a wide group the storing walker's cap beside its needle table, 42 496 bytes, needle or not
                const uint32_t rx_cap = wide_mix ? bsh_rtg::wide_regex_table_cap(bsh_rtg::with(mix, query_mix), false, group_cap)
                                                 : bsh_rtg::regex_table_cap(bsh_rtg::with(mix, query_mix), wide, false, group_cap);
                const bool fits = bsh_rtg::joins(mix_ok, mix, query_mix) && mp.kinds.size() <= cond_cap && index.size() + added.size() <= cond_cap && n_rx + fresh_rx <= bsh_rxg::kMaxRegexConds &&
                                  bsh_rxg::align4(rx_table + fresh_bytes) <= rx_cap &&
                                  bsh_rxg::co_active_bound(rx_fields) <= bsh_rxg::kManySlots &&
                                  (!needle_group || bsh_subg::fits(sub_group, fresh_sub, wide));   // the needles pack, the tables fit beside them
                if (!fits) {
                    // alone beyond the call: the caller's (the host matcher; per query for a regex query).  Else it opens the next group
                    if (members.empty()) ++pos;
                    break;
                }
                for (uint32_t op : mp.prog_ops) {
                    if ((op >> 28) == BSG_OP_TERM) {
                        const uint32_t c = op & 0x0FFFFFFFu;
                        auto it = index.emplace(std::make_tuple(mp.kinds[c], mp.fields[c], mp.tokens[c]), (uint32_t)kinds.size());
                        if (it.second) { kinds.push_back(mp.kinds[c]); fields.push_back(mp.fields[c]); tokens.push_back(mp.tokens[c]); }
                        op = BSG_OP(BSG_OP_TERM, it.first->second);
                    }
                    prog_ops.push_back(op);
                }
                prog_off.push_back((uint32_t)prog_ops.size());
                members.push_back(k);
                n_rx += fresh_rx;
                rx_table += fresh_bytes;
                n_plain += fresh_plain;
                n_ft += fresh_ft;
                bsh_subg::add(sub_group, fresh_sub);
                bsh_rngg::add(mix, query_mix);
            }
            if (members.empty()) continue;
            const bsh_subg::Call call = bsh_subg::group_call(n_rx != 0, sub_group.n_needles != 0, wide, wide_rows);
            const bool by_sub = sub_group.n_needles != 0, by_range = mix.range;
            const bool by_mixed = bsh_rtg::mixed(mix);           // kind 6 beside a text condition: only where mix_ok; under a wide key only with DeviceMatchRangeTextWide
            const char *call_name = wide && by_mixed ? bsh_rtg::wide_group_call_name(mix, n_rx != 0, by_sub, wide_rows)
                                                     : bsh_rtg::group_call_name(mix, n_rx != 0, by_sub, wide, wide_rows);   // (of a group no lookup call decides)
            // a row the device handed back: the host matchers of query m together
            auto host_verdict = [&](size_t m, const std::string &row) {
                return host_matchers[m].match(row) && (!host_regex[m] || host_regex[m]->match(row)) && (!host_sub[m] || host_sub[m]->match(row)) &&
                       (!host_range[m] || host_range[m]->match(row));
            };
            std::vector<uint8_t> cbytes;
            std::vector<uint32_t> coff{0};
            for (size_t c = 0; c < kinds.size(); ++c) {
                cbytes.insert(cbytes.end(), fields[c].begin(), fields[c].end()); coff.push_back((uint32_t)cbytes.size());
                cbytes.insert(cbytes.end(), tokens[c].begin(), tokens[c].end()); coff.push_back((uint32_t)cbytes.size());
            }
            if (wide) {
                const bool by_lookup = lookup && n_rx == 0 && !by_sub && !by_range, by_lookup_regex = lookup_regex && n_rx != 0 && !by_sub && !by_range;
                // each set's list: the group's members that survived the probe on it, straight from set_wants
                std::vector<uint32_t> sq_off{0}, sq;
                for (size_t s = 0; s < n_sets; ++s) {
                    for (size_t j = 0; j < members.size(); ++j)
                        if ((*set_wants[s])[members[j]]) sq.push_back((uint32_t)j);
                    sq_off.push_back((uint32_t)sq.size());
                }
                std::vector<uint64_t> pair_word_off(sq.size() + 1);
                uint64_t total = 0;
                if (bsg_match_wide_size(set_first.data(), sq_off.data(), (uint32_t)n_sets, (uint32_t)scan.size(), (uint32_t)members.size(),
                                        pair_word_off.data(), &total))
                    return fail(kErrGpu, bsg_last_error(ctx_));
                std::vector<uint32_t> fb(scan.size());
                uint32_t n_fb = 0;
                if (hist) {
                    // counts instead of rows: buckets + 3 per (set, listed query), summed per query; a handed-back row is matched by the
                    // host matchers per query listed on its set and bucketed by hist_row_slot (no JSON object: missing)
                    const size_t slots = (size_t)hist->buckets + 3;
                    std::vector<uint32_t> counts(sq.size() * slots + 1);
                    const int32_t rc = bsg_match_rows_wide_hist(ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(), kinds.data(),
                                                                (uint32_t)kinds.size(), prog_ops.data(), prog_off.data(), (uint32_t)members.size(), set_first.data(),
                                                                sq_off.data(), sq.data(), (uint32_t)n_sets, &tok, (const uint8_t *)hist->field.data(),
                                                                (uint32_t)hist->field.size(), hist->origin, hist->width, hist->buckets, counts.data(), fb.data(),
                                                                (uint32_t)fb.size(), &n_fb);
                    if (rc == BSG_E_UNSUPPORTED) continue;
                    if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
                    count_match_call("bsg_match_rows_wide_hist");
                    for (size_t p = 0; p < sq.size(); ++p) {
                        std::vector<uint64_t> &into = (*hist_counts)[members[sq[p]]];
                        for (size_t i = 0; i < slots; ++i) into[i] += counts[p * slots + i];
                    }
                    for (size_t j = 0; j < members.size(); ++j) on_device[members[j]] = 1;
                    for (uint32_t i = 0; i < n_fb; ++i) {
                        const size_t s = (size_t)(std::upper_bound(set_first.begin() + 1, set_first.end(), fb[i]) - (set_first.begin() + 1));
                        const std::string &row = *scan[fb[i]];
                        uint32_t slot = hist->buckets + 2u;
                        if (!hist_row_slot(row, hist->field, hist->origin, hist->width, hist->buckets, slot)) slot = hist->buckets + 2u;
                        for (uint32_t p = sq_off[s]; p < sq_off[s + 1]; ++p)
                            if (host_verdict(members[sq[p]], row)) ++(*hist_counts)[members[sq[p]]][slot];
                    }
                    continue;
                }
                if (wide_rows) {
                    // the lists themselves: 2 u32 per word is the payload's bound, so the call cannot fail on space
                    std::vector<uint32_t> hdr(sq.size() + 1), payload(2 * total + 1), ids;
                    std::vector<uint64_t> pair_off(sq.size() + 1);
                    uint64_t payload_len = 0;
                    count_match_call(by_lookup_regex ? "bsg_match_rows_lookup_regex_rows" : by_lookup ? "bsg_match_rows_lookup_rows" : call_name);
                    const int32_t rc = (by_lookup_regex ? bsg_match_rows_lookup_regex_rows : by_lookup ? bsg_match_rows_lookup_rows : by_mixed ? bsg_match_rows_wide_regex_substr_range_rows : by_sub ? bsg_match_rows_wide_substr_rows : by_range ? bsg_match_rows_wide_range_rows : bsg_match_rows_wide_rows)(ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(),
                                                                kinds.data(), (uint32_t)kinds.size(), prog_ops.data(), prog_off.data(),
                                                                (uint32_t)members.size(), set_first.data(), sq_off.data(), sq.data(), (uint32_t)n_sets, &tok,
                                                                hdr.data(), pair_off.data(), payload.data(), 2 * total, &payload_len, fb.data(),
                                                                (uint32_t)fb.size(), &n_fb);
                    if (rc == BSG_E_UNSUPPORTED) continue;
                    if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
                    for (size_t s = 0; s < n_sets; ++s) {
                        const uint32_t set_rows = set_first[s + 1] - set_first[s];
                        ids.resize(set_rows);
                        for (uint32_t p = sq_off[s]; p < sq_off[s + 1]; ++p) {
                            uint32_t n = 0;
                            if (bsg_match_pair_rows_list(hdr[p], payload.data() + pair_off[p], set_rows, ids.data(), set_rows, &n))
                                return fail(kErrGpu, bsg_last_error(ctx_));
                            uint8_t *h = hit[members[sq[p]]].data() + set_first[s];
                            std::fill(h, h + set_rows, (uint8_t)0);
                            for (uint32_t k = 0; k < n; ++k) h[ids[k]] = 1;
                        }
                    }
                } else {
                std::vector<uint64_t> words(total + 1);
                count_match_call(by_lookup_regex ? "bsg_match_rows_lookup_regex" : by_lookup ? "bsg_match_rows_lookup" : call_name);
                const int32_t rc = (by_lookup_regex ? bsg_match_rows_lookup_regex : by_lookup ? bsg_match_rows_lookup : by_mixed ? bsg_match_rows_wide_regex_substr_range : by_sub ? bsg_match_rows_wide_substr : by_range ? bsg_match_rows_wide_range : bsg_match_rows_wide)(ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(), kinds.data(),
                                                       (uint32_t)kinds.size(), prog_ops.data(), prog_off.data(), (uint32_t)members.size(), set_first.data(),
                                                       sq_off.data(), sq.data(), (uint32_t)n_sets, &tok, words.data(), fb.data(), (uint32_t)fb.size(), &n_fb);
                if (rc == BSG_E_UNSUPPORTED) continue;
                if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
                for (size_t s = 0; s < n_sets; ++s)
                    for (uint32_t p = sq_off[s]; p < sq_off[s + 1]; ++p) {
                        std::vector<uint8_t> &h = hit[members[sq[p]]];
                        const uint64_t *w = words.data() + pair_word_off[p];
                        for (uint32_t i = set_first[s]; i < set_first[s + 1]; ++i) h[i] = (w[(i - set_first[s]) >> 6] >> ((i - set_first[s]) & 63)) & 1;
                    }
                }
                for (size_t j = 0; j < members.size(); ++j) on_device[members[j]] = 1;
                for (uint32_t i = 0; i < n_fb; ++i) {           // per query listed on the row's set
                    const size_t s = (size_t)(std::upper_bound(set_first.begin() + 1, set_first.end(), fb[i]) - (set_first.begin() + 1));
                    const std::string &row = *scan[fb[i]];
                    for (uint32_t p = sq_off[s]; p < sq_off[s + 1]; ++p) {
                        const size_t m = members[sq[p]];
                        hit[m][fb[i]] = host_verdict(m, row);
                    }
                }
                continue;
            }
            std::vector<uint64_t> masks(n_sets, 0);
            for (size_t s = 0; s < n_sets; ++s)
                for (size_t j = 0; j < members.size(); ++j) masks[s] |= (uint64_t)((*set_wants[s])[members[j]] != 0) << j;
            std::vector<uint64_t> bits(members.size() * n_words);
            std::vector<uint32_t> fb(scan.size());
            uint32_t n_fb = 0;
            count_match_call(call_name);
            const int32_t rc = (by_mixed ? bsg_match_rows_many_regex_substr_range : by_range ? bsg_match_rows_many_range : call == bsh_subg::Call::ManyRegexSubstr ? bsg_match_rows_many_regex_substr : call == bsh_subg::Call::ManySubstr ? bsg_match_rows_many_substr :
                                n_rx ? bsg_match_rows_many_regex : bsg_match_rows_many)(
                ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(), kinds.data(), (uint32_t)kinds.size(),
                prog_ops.data(), prog_off.data(), (uint32_t)members.size(), set_first.data(), masks.data(), (uint32_t)n_sets, &tok, bits.data(),
                fb.data(), (uint32_t)fb.size(), &n_fb);
            if (rc == BSG_E_UNSUPPORTED) continue;              // programs too deep / long, tables too large: the caller decides
            if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
            for (size_t j = 0; j < members.size(); ++j) {
                std::vector<uint8_t> &h = hit[members[j]];
                for (size_t i = 0; i < scan.size(); ++i) h[i] = (bits[j * n_words + (i >> 6)] >> (i & 63)) & 1;
                on_device[members[j]] = 1;
            }
            for (uint32_t i = 0; i < n_fb; ++i) {               // rows outside the walker's envelope, colliding or over the slots: per live query
                const size_t s = (size_t)(std::upper_bound(set_first.begin() + 1, set_first.end(), fb[i]) - (set_first.begin() + 1));
                const std::string &row = *scan[fb[i]];
                for (size_t j = 0; j < members.size(); ++j)
                    if ((masks[s] >> j) & 1)
                        hit[members[j]][fb[i]] = host_verdict(members[j], row);
            }
        }
        return kEngineOk;
    }

    // The five single-query device matchers below differ in their program prologue, the entry point and the host matchers that decide
    // a row the device hands back (the walker's envelope, a fingerprint collision, ...): mp over the scan list in one call of `call`.
    // done stays false (the host decides) beyond 64 conditions or what the call holds (depth, ops, tables): BSG_E_UNSUPPORTED.
    // count_first: the call is counted before it is made; else only once it has not answered BSG_E_UNSUPPORTED.
    using MatchRowsCall = int32_t (*)(bsg_ctx *, const uint8_t *, const uint64_t *, uint32_t, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t,
                                      const uint32_t *, uint32_t, const bsg_tokenizer *, uint64_t *, uint32_t *, uint32_t, uint32_t *);
    template <class Fallback>
    int32_t match_program_on_device(const MatcherProgram &mp, MatchRowsCall call, const char *name, bool count_first,
                                    const std::vector<const std::string *> &scan, Fallback &&host_decides, std::vector<uint8_t> &hit, bool &done)
    {
        if (mp.kinds.size() > 64) return kEngineOk;
        // condition strings as the C-ABI takes them: field i, token i, ... (hashed and fingerprinted on the device)
        std::vector<uint8_t> cbytes;
        std::vector<uint32_t> coff{0};
        for (size_t c = 0; c < mp.kinds.size(); ++c) {
            cbytes.insert(cbytes.end(), mp.fields[c].begin(), mp.fields[c].end()); coff.push_back((uint32_t)cbytes.size());
            cbytes.insert(cbytes.end(), mp.tokens[c].begin(), mp.tokens[c].end()); coff.push_back((uint32_t)cbytes.size());
        }
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> row_off{0};
        for (const std::string *r : scan) { bytes.insert(bytes.end(), r->begin(), r->end()); row_off.push_back(bytes.size()); }
        std::vector<uint64_t> bits((scan.size() + 63) / 64);
        std::vector<uint32_t> fb(scan.size());
        uint32_t n_fb = 0;
        const bsg_tokenizer tok = c_tokenizer();
        if (count_first) count_match_call(name);
        const int32_t rc = call(ctx_, bytes.data(), row_off.data(), (uint32_t)scan.size(), cbytes.data(), coff.data(), mp.kinds.data(), (uint32_t)mp.kinds.size(),
                                mp.prog_ops.data(), (uint32_t)mp.prog_ops.size(), &tok, bits.data(), fb.data(), (uint32_t)fb.size(), &n_fb);
        if (rc == BSG_E_UNSUPPORTED) return kEngineOk;
        if (!count_first) count_match_call(name);
        if (rc) return fail(kErrGpu, bsg_last_error(ctx_));
        for (size_t i = 0; i < scan.size(); ++i) hit[i] = (bits[i >> 6] >> (i & 63)) & 1;
        for (uint32_t i = 0; i < n_fb; ++i) hit[fb[i]] = host_decides(*scan[fb[i]]);
        done = true;
        return kEngineOk;
    }

    int32_t match_rows_device(const BloomExpression *expr, const std::vector<const std::string *> &scan, RowMatcher &host_matcher,
                              std::vector<uint8_t> &hit, bool &on_device)
    {
        const MatcherProgram mp(expr);
        return match_program_on_device(mp, bsg_match_rows_tok, "bsg_match_rows_tok", true, scan,
                                       [&](const std::string &row) { return host_matcher.match(row); }, hit, on_device);
    }

    // And(bloom root | TRUE, substring root) in one bsg_match_rows_substr call (128 needle bytes)
    int32_t match_rows_device_substr(const BloomExpression *expr, const SubstringExpression &sub, const std::vector<const std::string *> &scan,
                                     RowMatcher &host_matcher, SubstringRowMatcher &sub_matcher, std::vector<uint8_t> &hit, bool &done)
    {
        MatcherProgram mp(expr);
        if (mp.prog_ops.empty()) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        emit_substring_program(sub, mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
        mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 2));
        return match_program_on_device(mp, bsg_match_rows_substr, "bsg_match_rows_substr", true, scan,
                                       [&](const std::string &row) { return host_matcher.match(row) && sub_matcher.match(row); }, hit, done);
    }

    // And(bloom root | TRUE, range root) in one bsg_match_rows_range call (handed back as well: an exponent literal on a range field)
    int32_t match_rows_device_range(const BloomExpression *expr, const RangeExpression &range, const std::vector<const std::string *> &scan,
                                    RowMatcher &host_matcher, RangeRowMatcher &range_matcher, std::vector<uint8_t> &hit, bool &done)
    {
        MatcherProgram mp(expr);
        if (mp.prog_ops.empty()) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        emit_range_program(range, mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
        mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 2));
        return match_program_on_device(mp, bsg_match_rows_range, "bsg_match_rows_range", true, scan,
                                       [&](const std::string &row) { return host_matcher.match(row) && range_matcher.match(row); }, hit, done);
    }

    // And(bloom root | TRUE, regex root, substring root) in one bsg_match_rows_regex_substr call (the host's regex matcher DFA-backed,
    // as the device read the patterns)
    int32_t match_rows_device_regex_substr(const BloomExpression *expr, const RegexExpression &regex, const SubstringExpression &sub,
                                           const std::vector<const std::string *> &scan, RowMatcher &host_matcher, RegexRowMatcher &host_regex,
                                           SubstringRowMatcher &sub_matcher, std::vector<uint8_t> &hit, bool &done)
    {
        MatcherProgram mp(expr);
        if (mp.prog_ops.empty()) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        lower_regex(regex, mp);
        emit_substring_program(sub, mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
        mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 3));
        return match_program_on_device(mp, bsg_match_rows_regex_substr, "bsg_match_rows_regex_substr", true, scan,
                                       [&](const std::string &row) { return host_matcher.match(row) && host_regex.match(row) && sub_matcher.match(row); }, hit, done);
    }

    // And(bloom root | TRUE, regex root | TRUE, substring root | TRUE, range root) in one bsg_match_rows_regex_substr_range call
    // (device_match_range_text).  After BSG_E_UNSUPPORTED the route without the key decides, and only its calls are counted.
    int32_t match_rows_device_range_text(const BloomExpression *expr, const RegexExpression *regex, const SubstringExpression *sub, const RangeExpression &range,
                                         const std::vector<const std::string *> &scan, RowMatcher &host_matcher, RegexRowMatcher &host_regex,
                                         SubstringRowMatcher &sub_matcher, RangeRowMatcher &range_matcher, std::vector<uint8_t> &hit, bool &done)
    {
        MatcherProgram mp(expr);
        if (mp.prog_ops.empty()) mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        if (regex) lower_regex(*regex, mp); else mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        if (sub) emit_substring_program(*sub, mp.kinds, mp.fields, mp.tokens, mp.prog_ops); else mp.prog_ops.push_back(BSG_OP(BSG_OP_TRUE, 0));
        emit_range_program(range, mp.kinds, mp.fields, mp.tokens, mp.prog_ops);
        mp.prog_ops.push_back(BSG_OP(BSG_OP_AND, 4));
        return match_program_on_device(mp, bsg_match_rows_regex_substr_range, "bsg_match_rows_regex_substr_range", false, scan, [&](const std::string &row) {
            return host_matcher.match(row) && (!regex || host_regex.match(row)) && (!sub || sub_matcher.match(row)) && range_matcher.match(row);
        }, hit, done);
    }

    // Hand the stored section bytes to the device as they are: CRC32C + big-endian decode run in
    // k_decode_sections (bsg_arena_load_sections); the host never touches a filter word on the read path.
    int32_t load_arena(const std::vector<const std::vector<uint8_t> *> &sections, uint64_t &arena_id, std::vector<int32_t> &status)
    {
        std::vector<uint8_t> region;
        std::vector<uint64_t> off{0};
        for (auto *sec : sections) { region.insert(region.end(), sec->begin(), sec->end()); off.push_back(region.size()); }
        status.assign(std::max<size_t>(sections.size(), 1), 0);
        if (bsg_arena_load_sections(ctx_, region.data(), region.size(), off.data(), (uint32_t)sections.size(), status.data(), &arena_id))
            return fail(kErrGpu, bsg_last_error(ctx_));
        return kEngineOk;
    }

    int32_t ensure_files_arena()
    {
        if (files_arena_valid_) return kEngineOk;
        std::vector<const std::vector<uint8_t> *> fsec;
        for (auto &f : files_) fsec.push_back(&f.filter_section);
        if (int32_t rc = load_arena(fsec, files_arena_, file_status_)) return rc;
        files_arena_valid_ = true;
        return kEngineOk;
    }

    // Each distinct term is hashed once per query, on the device (bsg_hash_entries).
    int32_t hash_terms(const QueryBatch &qb, std::vector<bsg_term> &terms)
    {
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> offsets{0};
        for (auto &s : qb.term_strings) { bytes.insert(bytes.end(), s.begin(), s.end()); offsets.push_back((uint32_t)bytes.size()); }
        std::vector<uint64_t> h(qb.term_strings.size() * 4);
        if (!qb.term_strings.empty() &&
            bsg_hash_entries(ctx_, bytes.data(), offsets.data(), (uint32_t)qb.term_strings.size(), h.data()))
            return fail(kErrGpu, bsg_last_error(ctx_));
        terms.resize(qb.term_strings.size());
        for (size_t i = 0; i < terms.size(); ++i) {
            for (int j = 0; j < 4; ++j) terms[i].h[j] = h[i * 4 + j];
            terms[i].kind = qb.term_kinds[i];
            terms[i].reserved = 0;
        }
        return kEngineOk;
    }
};

}  // namespace bsh
