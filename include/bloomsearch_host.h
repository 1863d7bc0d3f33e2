/*
 * bloomsearch_host.h — C-ABI of the host-side mirror that sits ABOVE bloomgpu.h.
 *
 * The reference's host is Go; this image has no Go toolchain, so the host side of the path is
 * written in C++ (bloomsearch_amd/csrc/host/) mirroring the reference's own functions, and exposed
 * here so tests (and any embedding) can drive it.  A Go host does NOT need this header: it keeps its
 * own tokenizer.go / ingest.go / query.go and binds bloomgpu.h directly.
 *
 * Mirrors (reference file:line):
 *   bsh_tokenize ............. BasicWhitespaceLowerTokenizer, tokenizer.go:141-143
 *   bsh_tokenize_with ........ strings.FieldsFunc(lower ? strings.ToLower(v) : v, isSep) (the separator family)
 *   bsh_entry_sets_* ......... bloomEntrySets.indexRow/unionInto/counts, ingest.go:24-123
 *   bsh_batch_* .............. Field/Token/FieldToken/And/Or trees (JSON of the exported structs,
 *                              query.go:478-610) lowered to bloomgpu.h terms + programs
 *   bsh_match_row ............ testJSONForBloomQuery / compiledRowMatcher, row_matcher.go:486-626
 *   bsh_section_* ............ encodeFilterSection / parseFilterSection, file_format.go:343-448
 *   bse_* .................... BloomSearchEngine IngestRows / Flush / Query / Merge
 *                              (ingest.go:170,197; query_exec.go:201; merge.go:35)
 * All functions return 0 on success or a negative code; buffers returned through `char **` are
 * malloc'd and released with bsh_free.
 */
#ifndef BLOOMSEARCH_HOST_H
#define BLOOMSEARCH_HOST_H

#include <stdint.h>
#include "bloomgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSH_E_INVALID        -1
#define BSE_E_INVALID_CONFIG -101  /* ErrInvalidConfig */
#define BSE_E_ENGINE_STOPPED -102  /* ErrEngineStopped */
#define BSE_E_INVALID_ROW    -103
#define BSE_E_INVALID_QUERY  -104
#define BSE_E_GPU            -105
#define BSE_E_INVALID_HASH   -106  /* ErrInvalidHash */

BSG_API void bsh_free(void *p);

/* tokens of `text`, joined by '\n' (a token never contains white space) */
BSG_API int32_t bsh_tokenize(const uint8_t *text, uint64_t len, char **out, uint64_t *out_len);
/* tokens of `text` under a tokenizer of the separator family (bloomgpu.h bsg_tokenizer; NULL = the default), packed as
 * (u32 little-endian length, bytes) per token: such a token may hold any byte but a separator.  A spec with an n-gram width
 * (BSG_TOK_NGRAM) gives each word's windows in order.  BSH_E_INVALID for an invalid spec (a width of 1 or above 4 included). */
BSG_API int32_t bsh_tokenize_with(const uint8_t *text, uint64_t len, const bsg_tokenizer *tok, uint8_t **out, uint64_t *out_len);

typedef struct bsh_entry_sets bsh_entry_sets;
BSG_API bsh_entry_sets *bsh_entry_sets_new(void);
BSG_API void bsh_entry_sets_free(bsh_entry_sets *s);
/* indexRow on one marshaled-JSON row; BSH_E_INVALID if it is not valid JSON */
BSG_API int32_t bsh_entry_sets_index_row(bsh_entry_sets *s, const uint8_t *row, uint64_t len);
/* indexRow with the words of a separator-family tokenizer (NULL = the default); BSH_E_INVALID for an invalid spec too */
BSG_API int32_t bsh_entry_sets_index_row_with(bsh_entry_sets *s, const uint8_t *row, uint64_t len, const bsg_tokenizer *tok);
BSG_API int32_t bsh_entry_sets_union_into(const bsh_entry_sets *src, bsh_entry_sets *dst);
BSG_API void bsh_entry_sets_counts(const bsh_entry_sets *s, uint64_t counts[3]);
/* packed export of one kind (0 field, 1 token, 2 field::token): sizes, then fill */
BSG_API int32_t bsh_entry_sets_export_sizes(const bsh_entry_sets *s, uint32_t kind, uint64_t *n_entries, uint64_t *n_bytes);
BSG_API int32_t bsh_entry_sets_export(const bsh_entry_sets *s, uint32_t kind, uint8_t *bytes, uint32_t *offsets);

typedef struct bsh_batch bsh_batch;
BSG_API bsh_batch *bsh_batch_new(void);
BSG_API void bsh_batch_free(bsh_batch *b);
/* expression JSON in the reference's struct shape; "null" / empty = nil query */
BSG_API int32_t bsh_batch_add_query(bsh_batch *b, const char *expr_json, uint64_t len);
BSG_API void bsh_batch_sizes(const bsh_batch *b, uint32_t *n_queries, uint32_t *n_terms, uint32_t *n_ops, uint64_t *term_bytes);
BSG_API int32_t bsh_batch_export(const bsh_batch *b, uint8_t *term_bytes, uint32_t *term_offsets, uint32_t *term_kinds,
                                 uint32_t *prog_ops, uint32_t *prog_off);

/* final exact test of one row against one expression: 1 match, 0 no match, negative error */
BSG_API int32_t bsh_match_row(const char *expr_json, uint64_t expr_len, const uint8_t *row, uint64_t row_len);
/* the same under a separator-family tokenizer (bloomgpu.h bsg_tokenizer; NULL = the default): the host matcher the rows
 * bsg_match_rows_tok hands back are decided by.  BSH_E_INVALID for an invalid spec. */
BSG_API int32_t bsh_match_row_with(const char *expr_json, uint64_t expr_len, const uint8_t *row, uint64_t row_len, const bsg_tokenizer *tok);
/* pruneBloomQuery = AndBloomQueries(bloom, RegexFieldGuardBloomQuery(regex)) (query_exec.go:220, query.go:651-718) as JSON in the
 * reference's struct shape; "null" when both sides are nil.  regex_json: {"ExpressionType": "CONDITION"|"AND"|"OR",
 * "Condition": {"Field", "Pattern"}, "Children": [...]}. */
BSG_API int32_t bsh_prune_query(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len, char **out, uint64_t *out_len);
/* The regex half of the final row test (row_matcher.go:548-573; std::regex ECMAScript stands in for RE2): 1 / 0 / < 0. */
BSG_API int32_t bsh_match_row_regex(const char *regex_json, uint64_t regex_len, const uint8_t *row, uint64_t row_len);

/* ---- substring conditions (bloomgpu.h "substring conditions"; bloomsearch_amd/csrc/host/substring.hpp) ----
 * substring_json: {"ExpressionType": "CONDITION"|"AND"|"OR", "Condition": {"Field": string or absent, "Needle": string},
 * "Children": [...]}; a condition without "Field" looks at every leaf, one with it at the leaves whose path equals the field.
 * A needle is non-empty valid UTF-8 of at most 64 bytes after folding: BSH_E_INVALID (empty, invalid UTF-8, an invalid spec or
 * JSON) or BSG_E_UNSUPPORTED (too long) otherwise.  tok: the tokenizer of the store (NULL = the default). */
/* the pruning terms of one needle, packed as bsh_tokenize_with packs tokens, deduplicated in first-occurrence order */
BSG_API int32_t bsh_substring_terms(const uint8_t *needle, uint64_t len, const bsg_tokenizer *tok, uint8_t **out, uint64_t *out_len);
/* bsh_prune_query with the third tree: And(bloom, regex field guard, substring guard) as JSON, "null" when every side is nil.  A
 * condition's guard is And(Token(t) ..) / And(FieldToken(field, t) ..) over its terms; without terms Field(field), or for an
 * any-field condition the nil condition ({"ExpressionType":"CONDITION","Condition":null}: always true), which an And drops and an
 * Or keeps.  A NULL / empty / "null" substring tree gives exactly bsh_prune_query's answer. */
BSG_API int32_t bsh_prune_query_sub(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len,
                                    const char *substring_json, uint64_t substring_len, const bsg_tokenizer *tok, char **out, uint64_t *out_len);
/* The substring half of the final row test: 1 when the tree holds for the row, 0 when not, < 0 as above (a row that is not
 * valid JSON: 0).  The matcher of the rows bsg_match_rows_substr hands back. */
BSG_API int32_t bsh_match_row_substring(const char *substring_json, uint64_t substring_len, const uint8_t *row, uint64_t row_len,
                                        const bsg_tokenizer *tok);
/* Range conditions (bloomgpu.h "Range conditions").  range_json: {"ExpressionType":"CONDITION"|"AND"|"OR","Condition":{"Field",
 * "Lo"?,"Hi"?,"LoOpen"?,"HiOpen"?},"Children":[..]} with int64 "Lo" / "Hi" (absent or null: unbounded; anything else: < 0).
 * The range half of the final row test: 1 when the tree holds for the row, 0 when not, < 0 for invalid arguments (a row that is not
 * valid JSON: 0).  Exact for every JSON number literal, exponents included: the literal's digits are compared with the bound's, no
 * floating point.  The matcher of the rows bsg_match_rows_range hands back. */
BSG_API int32_t bsh_match_row_range(const char *range_json, uint64_t range_len, const uint8_t *row, uint64_t row_len);
/* bsh_prune_query_sub with the fourth tree: And(bloom, regex field guard, substring guard, range guard).  A range condition's guard
 * is Field(field); the nil condition is dropped from an And and kept in an Or, as in the substring guard.  A NULL / empty / "null"
 * range tree gives exactly bsh_prune_query_sub's answer. */
BSG_API int32_t bsh_prune_query_range(const char *bloom_json, uint64_t bloom_len, const char *regex_json, uint64_t regex_len,
                                      const char *substring_json, uint64_t substring_len, const char *range_json, uint64_t range_len,
                                      const bsg_tokenizer *tok, char **out, uint64_t *out_len);

/* ---- MinMax indexes (bloomgpu.h "per-set MinMax indexes"; bloomsearch_amd/csrc/host/minmax.hpp) ----
 * One row's contributions folded into inout[n_fields] (fields packed as for bsg_ingest_rows_minmax; an index with present == 0 is
 * absent and takes the first contribution as it is).  Exact for EVERY number literal, exponents of any size included
 * (1e99999999999999999999 gives (INT64_MAX, INT64_MAX)); escaped keys are decoded; the last duplicate wins; no floating point.
 * The function the rows a device ingest hands back are folded in with.  BSH_E_INVALID: invalid fields, or a row that is not one
 * valid JSON object (nothing is folded). */
BSG_API int32_t bsh_minmax_row(const uint8_t *row, uint64_t len, const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields,
                               bsg_minmax *inout);
/* One row's slot among the BSG_HIST_SLOTS(n_buckets) of bsg_match_rows_wide_hist (bloomgpu.h "Bucketed hit counts"): a bucket, or
 * n_buckets (below), n_buckets + 1 (above), n_buckets + 2 (missing).  The field, the row's value t = clamp(floor(v)) and the bucket
 * rule are that call's; exact for EVERY number literal, exponents included, and escaped keys are decoded (built on bsh_minmax_row's
 * scan): the function the rows that call hands back are bucketed with.  BSH_E_INVALID: a name of 0 or more than BSG_MINMAX_MAX_NAME
 * bytes, width 0, n_buckets 0 or above BSG_HIST_MAX_BUCKETS, null pointers, or a row that is not one valid JSON object. */
BSG_API int32_t bsh_hist_row(const uint8_t *row, uint64_t len, const uint8_t *field, uint32_t field_len, int64_t origin, uint64_t width,
                             uint32_t n_buckets, uint32_t *out_slot);
/* One row's partition text by the rule of the keyed ingest (bloomgpu.h "keyed streaming ingest"; the engine's PartitionField): the
 * FIRST top-level member whose decoded key equals name[name_len] (1 to BSG_PARTITION_MAX_NAME bytes) gives a string's decoded
 * bytes, a number's raw literal, "true" or "false"; null, an object, an array or no such member give the empty text.  Exact for
 * EVERY row, escapes in keys and values decoded: the function the rows a keyed ingest hands back are decided with.  *out_len = the
 * text's length; its first min(cap, *out_len) bytes are written to out (a text is never longer than its row).  BSH_E_INVALID: an
 * empty or over-long name, null pointers, or a row that is not one valid JSON object. */
BSG_API int32_t bsh_partition_key(const uint8_t *row, uint64_t len, const uint8_t *name, uint32_t name_len, uint8_t *out, uint64_t cap,
                                  uint64_t *out_len);
/* EvaluateMinMaxCondition (query.go) on a present index: 1 the block may hold a matching value, 0 it cannot.  A bound at an int64
 * extreme is saturated (the true value may lie beyond it): NE, GT, LT and NOT_BETWEEN keep such a block.  NOT_IN is always 1.
 * value: EQ NE GT GE LT LE; values[n_values]: IN; min, max: BETWEEN, NOT_BETWEEN.  BSH_E_INVALID: an absent index, an unknown op. */
#define BSH_MM_EQ 0u
#define BSH_MM_NE 1u
#define BSH_MM_GT 2u
#define BSH_MM_GE 3u
#define BSH_MM_LT 4u
#define BSH_MM_LE 5u
#define BSH_MM_IN 6u
#define BSH_MM_NOT_IN 7u
#define BSH_MM_BETWEEN 8u
#define BSH_MM_NOT_BETWEEN 9u
BSG_API int32_t bsh_minmax_eval(const bsg_minmax *index, uint32_t op, int64_t value, const int64_t *values, uint32_t n_values, int64_t min,
                                int64_t max);
/* evaluatePrefilterExpression (query.go) for one block.  prefilter_json: {"ExpressionType":"CONDITION"|"AND"|"OR","Condition":
 * {"ConditionType":"PARTITION"|"MINMAX","PartitionCondition":{"Operator":"EQ"|"NE"|"GT"|"GTE"|"LT"|"LTE"|"IN"|"NOT_IN"|"BETWEEN"|
 * "NOT_BETWEEN","Value","Values","Min","Max"},"MinMaxFieldName","MinMaxCondition":{the same with int64 operands}},"Children":[..]};
 * NULL / empty / "null": 1.  The block: its partition id and indexes[n_fields] named by the packed fields (present == 0: the block
 * does not carry that index).  An empty Or is 0, an empty And 1, a nil condition 1, a block without the named index 0, an empty
 * partition id fails every partition condition.  1 the block passes, 0 it does not, BSH_E_INVALID for invalid arguments. */
BSG_API int32_t bsh_prefilter_eval(const char *prefilter_json, uint64_t len, const uint8_t *partition_id, uint64_t partition_len,
                                   const uint8_t *field_bytes, const uint32_t *field_off, uint32_t n_fields, const bsg_minmax *indexes);

/* Go regexp MatchString of `pattern` on `text` for the subset the device row matcher compiles (bsg_match_rows_regex; the
 * subset is listed in bloomsearch_amd/csrc/host/regex_dfa.hpp), run on the same DFA tables.  The text is read as Go reads a
 * string: an invalid byte is U+FFFD.  1 match, 0 no match, BSG_E_UNSUPPORTED for a pattern outside the subset (syntax
 * errors included), BSH_E_INVALID for null pointers. */
BSG_API int32_t bsh_regex_match(const char *pattern, uint64_t plen, const uint8_t *text, uint64_t tlen);

/* filter section codec; filters[c].m == 0 => absent */
BSG_API int32_t bsh_section_encode(const uint64_t *const words[3], const uint64_t m[3], const uint64_t k[3],
                                   uint8_t **out, uint64_t *out_len);
/* on success fills m/k and returns each present filter's words (malloc'd, native LE) */
BSG_API int32_t bsh_section_parse(const uint8_t *section, uint64_t len, uint64_t m[3], uint64_t k[3], uint64_t *words[3]);
BSG_API uint32_t bsh_crc32c(const uint8_t *data, uint64_t len);

/* ---- engine mirror ---- */
typedef struct bse_engine bse_engine;
/* config_json: {"MaxRowGroupRows":..,"MaxRowGroupBytes":..,"MaxBufferedRows":..,"MaxBufferedBytes":..,
 *               "BloomFalsePositiveRate":..,"PartitionField":"..","DeviceIngest":true|false,"DeviceIngestStream":true|false,
 *               "TrustedRows":true|false,"DevicePartition":true|false,"DeviceMatch":true|false,
 *               "DeviceRegex":true|false,"DeviceMatchRangeText":true|false,"DeviceMatchWide":true|false,"DeviceMatchWideRows":true|false,
 *               "DeviceMatchRangeTextWide":true|false,"DeviceMatchHistogram":true|false,
 *               "DeviceMatchLookup":true|false,"DeviceMatchLookupRows":true|false,"DeviceMatchLookupRegex":true|false,
 *               "Tokenizer":{"Separators":"..","UnicodeSpace":true|false,"Lower":true|false,"Ngram":0|2|3|4},
 *               "MinMaxIndexes":["timestamp",..]};
 *               missing keys take the
 *               reference defaults.  DeviceIngest (default false): rows are walked / tokenized / deduplicated /
 *               counted on the GPU at flush and merge time (bloomgpu.h bsg_ingest_*) instead of by indexRow on the
 *               host at ingest time; the files it writes are byte-identical either way.  DeviceIngestStream (default false,
 *               needs DeviceIngest: BSE_E_INVALID_CONFIG without it): every bse_ingest_rows batch is handed to an open
 *               streaming ingest when it arrives (bsg_ingest_open / _add_sets / _append_rows) and its fallback rows are
 *               finished at once, so a flush only finishes, sizes and builds; merge keeps the one-shot path; same bytes.
 *               TrustedRows (default false): the caller promises one valid JSON object per row (the reference marshals its own
 *               rows, ingest.go:379-396); bse_ingest_rows then validates no row for its own sake.  DevicePartition (default
 *               false; needs DeviceIngestStream, TrustedRows and a non-empty PartitionField of at most 64 bytes:
 *               BSE_E_INVALID_CONFIG otherwise): every batch goes to a KEYED streaming ingest (bsg_ingest_open_keyed /
 *               _append_rows_keyed), the device finds each row's partition, and only the rows it hands back are parsed on the
 *               host (bsh_partition_key's rule); same files, same bytes.
 *               DeviceMatch (default false): the
 *               final row test of the surviving blocks runs on the GPU (bsg_match_rows) instead of in the host matcher;
 *               the delivered row set is the same.  DeviceMatchWide (default false, needs DeviceMatch): bse_query_many packs
 *               its queries into groups bounded by 64 distinct conditions (16 regex), not by 64 members, and decides each
 *               group by one bsg_match_rows_wide call; same answers.  DeviceMatchWideRows (default false, needs DeviceMatch):
 *               the same groups, each decided by one bsg_match_rows_wide_rows call whose row lists are consumed as they
 *               come, no bit row is scanned; same answers.  DeviceMatchLookup / DeviceMatchLookupRows (default false, need
 *               DeviceMatch): the groups of DeviceMatchWide / DeviceMatchWideRows, but a group without a regex condition
 *               holds up to 1 024 distinct conditions and is decided by one bsg_match_rows_lookup / _lookup_rows call (the
 *               table arithmetic: csrc/host/lookup_plan.hpp, beside wide_plan.hpp); queries with a regex condition keep
 *               their 64-condition groups and the wide call; same answers.  DeviceMatchLookupRegex (default false, acts with
 *               DeviceMatchLookup or DeviceMatchLookupRows, and DeviceRegex): a group WITH regex conditions keeps the 1 024
 *               conditions too and is decided by one bsg_match_rows_lookup_regex / _lookup_regex_rows call; it closes at 16
 *               regex conditions, at more than 4 of them over one leaf, and where their tables pass what the group's strings
 *               (<= 2 x its other conditions) and pairs (<= its FieldToken conditions) leave of the walker's LDS
 *               (lookup_plan.hpp rx_lds_cap_of); same answers.  DeviceRegex (default false, needs DeviceMatch):
 *               a query whose regex patterns all lie in the device's RE2 subset is matched bloom AND regex by one
 *               bsg_match_rows_regex call, the rows it hands back by the host matcher on the same DFAs; other regex queries
 *               keep the std::regex path.  DeviceMatchRangeText (default false, needs DeviceMatch): bse_query decides a
 *               query that has a Range tree beside a Regex and / or Substring tree by one bsg_match_rows_regex_substr_range
 *               call (a Regex tree takes part only under DeviceRegex with every pattern in the device subset; where the
 *               library answers BSG_E_UNSUPPORTED the query takes the route it takes without the key; a Regex tree outside
 *               the subset is left to the host matcher and the call decides range and substring); same answers.  With no wide
 *               or lookup key set, bse_query_many lets such queries share its groups with range-only and text-only ones: a
 *               group whose table holds a range condition beside a regex or substring one makes one
 *               bsg_match_rows_many_regex_substr_range call (64 queries, 64 conditions, 16 regex conditions, needles that pack,
 *               regex tables of at most 34 032 bytes); under a wide or lookup key groups never mix without the next key.
 *               DeviceMatchRangeTextWide (default false; needs DeviceMatch, DeviceMatchRangeText and at least one of
 *               DeviceMatchWide, DeviceMatchWideRows, DeviceMatchLookup, DeviceMatchLookupRows: BSE_E_INVALID_CONFIG otherwise):
 *               under those keys too bse_query_many lets range and text conditions share a group: a wide group (no member limit,
 *               64 conditions, 16 regex conditions, needles that pack, regex tables of at most 42 496 bytes needle or not) whose
 *               table holds both makes one bsg_match_rows_wide_regex_substr_range call, under a rows key one
 *               bsg_match_rows_wide_regex_substr_range_rows call, and never a lookup call; bse_query is unchanged; same answers.
 *               DeviceMatchHistogram (default false; needs DeviceMatch and one of DeviceMatchWide, DeviceMatchWideRows:
 *               BSE_E_INVALID_CONFIG otherwise): in bse_query_many the queries that carry a "Histogram" member leave the batch's
 *               groups; those with an equal spec form wide groups of their own (the wide groups' closing rules, 64 conditions),
 *               each decided by ONE bsg_match_rows_wide_hist call: per-set counts summed per query on the host, the rows the call
 *               hands back matched by the host matchers and bucketed by bsh_hist_row's rule; BSG_E_UNSUPPORTED and a query outside
 *               a group take the host route.  Without the key, and always in bse_query, a "Histogram" query is matched as any
 *               query and every matching row bucketed on the host.  Same answers on both routes.
 *               Tokenizer (default: BasicWhitespaceLowerTokenizer): the engine's tokenizer
 *               of the separator family (bloomgpu.h bsg_tokenizer), used by indexing, the host matcher and the device calls;
 *               a missing member is Go's zero value ("" / false); BSE_E_INVALID_CONFIG for a NUL or non-ASCII separator.
 *               MinMaxIndexes (default none): top-level keys whose per-block [min, max] every flush records (bloomgpu.h "per-set
 *               MinMax indexes": 1 to 8 distinct names of 1 to 64 bytes, BSE_E_INVALID_CONFIG otherwise).  Without DeviceIngest
 *               every row is folded by bsh_minmax_row at ingest time; with DeviceIngest / DeviceIngestStream the flush's device
 *               call computes the indexes (bsg_ingest_rows_minmax / bsg_ingest_open_minmax) and only the rows it hands back are
 *               folded on the host; the indexes are the same on every route.  Merge joins two blocks of a partition only when
 *               their index KEY SETS are equal (merge.go:208-260) and unions the sources' indexes.
 *               The config is checked before ctx: an invalid one gives BSE_E_INVALID_CONFIG even with a NULL ctx, a valid one
 *               with a NULL ctx BSH_E_INVALID. */
BSG_API int32_t bse_open(const char *config_json, uint64_t len, bsg_ctx *ctx, bse_engine **out);
BSG_API void bse_close(bse_engine *e);
BSG_API const char *bse_last_error(bse_engine *e);
BSG_API int32_t bse_stop(bse_engine *e);
/* rows: marshaled JSON objects separated by '\n' */
BSG_API int32_t bse_ingest_rows(bse_engine *e, const uint8_t *ndjson, uint64_t len);
BSG_API int32_t bse_flush(bse_engine *e);
BSG_API int32_t bse_merge(bse_engine *e);
/* query_json: {"Bloom":{"Expression":{...}}} (or {"Bloom":null}), with optional "Regex", "Substring" and "Range" trees (the last:
 * bsh_match_row_range's tree, or {"Expression": tree}; under DeviceMatch a query with a Range tree and neither of the other two is
 * decided by ONE bsg_match_rows_range call over And(bloom, range)); result JSON:
 * An optional "Prefilter": {"Expression": tree} (bsh_prefilter_eval's tree) is applied to every block's partition id and MinMax
 * indexes: a block failing it is neither scanned nor given a BlockStats entry, and a file left without blocks counts in neither
 * FilesConsidered nor FilesBloomSkipped; in bse_query_many every query has its own prefilter, and a block no query keeps is not
 * walked.  A query without a Prefilter takes exactly the path it took before.  Result JSON:
 * {"rows":[...],"stats":{"BlockStats":[{"FileID","BlockOffset","RowsProcessed","BytesProcessed","TotalRows",
 *  "TotalBytes","BloomFilterSkipped"}],"Errors":[..],"FilesConsidered","FilesBloomSkipped"}} */
BSG_API int32_t bse_query(bse_engine *e, const char *query_json, uint64_t len, char **out_json, uint64_t *out_len);
/* A batch of queries in one pass.  queries_json: a JSON array of bse_query's query objects; out_json: a JSON array of bse_query's
 * result objects, element i equal to what bse_query returns for query i alone (rows in the same order, the same BlockStats,
 * Errors, FilesConsidered, FilesBloomSkipped; Duration is exempt).  All bloom-only queries share one query batch: one file-stage
 * probe, one bsg_probe_many over the leased arenas, then the rows of every block at least one query survived on are scanned once
 * - under DeviceMatch by one bsg_match_rows_many call per group of <= 64 queries / <= 64 distinct conditions, each block a set
 * with the mask of the queries that survived on it.  Under DeviceMatch + DeviceRegex a query with a Regex tree whose patterns
 * all lie in the device's RE2 subset joins the batch (probed with its pruning expression, matched by bsg_match_rows_many_regex in
 * groups of <= 16 regex conditions whose tables fit the batched kernel and of which no more than 4 can meet on one leaf); every
 * other query with a Regex tree is answered as by bse_query.  Under DeviceMatch a query with a "Substring" tree whose needles are
 * valid joins the batch too (with a Regex tree as well: under the rule above): it is probed with And(bloom, regex field guard,
 * substring guard) and matched as And(bloom | TRUE, regex, substring); a group that holds a needle also closes where the needles of
 * its distinct substring conditions no longer pack first-fit into 2 x 64 bytes and bounds its regex tables by the cap beside a needle
 * table (34 032 bytes batched, 42 496 wide), and is decided by ONE bsg_match_rows_many_substr / bsg_match_rows_many_regex_substr call -
 * under DeviceMatchWide / DeviceMatchWideRows (and the lookup keys, which never take a group with a needle) by ONE
 * bsg_match_rows_wide_substr / bsg_match_rows_wide_substr_rows call.  A query that breaks a limit alone, and a group the library
 * answers BSG_E_UNSUPPORTED for, are answered as by bse_query.  Without DeviceMatch a query with a Substring tree is answered as by
 * bse_query.  Under DeviceMatch a query with a "Range" tree and neither a Regex nor a Substring tree joins the batch as well: it is
 * probed with And(bloom, range guard) and matched as And(bloom | TRUE, range); a group never holds a range condition beside a regex or
 * substring condition (it closes where the next query would create that mix, in either order; plain queries go with both), and a group
 * with a range condition is decided by ONE bsg_match_rows_many_range call - under DeviceMatchWide / DeviceMatchWideRows (and the lookup
 * keys, which never take such a group) by ONE bsg_match_rows_wide_range / bsg_match_rows_wide_range_rows call.  A query with a Range
 * tree beside a Regex or Substring tree, and every query with a Range tree without DeviceMatch, is answered as by bse_query
 * (DeviceMatchRangeText, and under a wide or lookup key DeviceMatchRangeTextWide, keep such a query in the batch: bse_open).
 * "[]" gives "[]". */
BSG_API int32_t bse_query_many(bse_engine *e, const char *queries_json, uint64_t len, char **out_json, uint64_t *out_len);
/* {"files":[{"FileID","BloomEntryCounts":{..},"section_bytes","blocks":[{"PartitionID","Rows","BloomEntryCounts":{..},
 *  "BloomFalsePositiveRate","BloomFilterSize","filters":[{"m","k"}|null x3],"MinMaxIndexes":{"f":{"Min":..,"Max":..}}}]}],
 *  ("MinMaxIndexes" is omitted when the block has none)
 *  "IngestStream":{"Batches","Rows","HostRows","Flushes"}} — the last: DeviceIngestStream at work since bse_open: bse_ingest_rows
 *  batches and rows handed to a streaming ingest when they arrived, the rows among them the host walker finished at once, and the
 *  flushes built from a stream.  A batch whose append fails is answered with the error and is not buffered; the rows buffered
 *  before it are flushed through the one-shot path. */
BSG_API int32_t bse_describe(bse_engine *e, char **out_json, uint64_t *out_len);
/* {"bsg_match_rows_regex_substr": 3, "bsg_match_rows_tok": 1, ...}: how often the engine has called each device row-matcher entry
 * point (bloomgpu.h bsg_match_rows_*) since bse_open, a call the library answered BSG_E_UNSUPPORTED included; an entry point never
 * called is absent.  The route a query took: bsg_device_calls counts parts, and every route makes one match part. */
BSG_API int32_t bse_match_calls(bse_engine *e, char **out_json, uint64_t *out_len);
/* fault injection (the reference's tests wrap its stores to corrupt reads): XOR one byte of a stored section */
BSG_API int32_t bse_corrupt_section_byte(bse_engine *e, uint32_t file_index, int32_t block_index, uint64_t byte_index);
/* raw filter-section bytes of (file index, block index); block index -1 = the file-level section */
BSG_API int32_t bse_section_bytes(bse_engine *e, uint32_t file_index, int32_t block_index, uint8_t **out, uint64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
