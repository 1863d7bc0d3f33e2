// match_api.inc — C-ABI of the device row matcher (included by bloomgpu.hip).  Kernels: match.hip.h; host arithmetic: host/wide_plan.hpp.
// Every family (bsg_match_rows / _regex / _tok, bsg_match_rows_many / _many_regex, bsg_match_rows_wide, bsg_match_rows_lookup / _lookup_regex) takes ONE path:
//   entry point -> MatchCall (the caller's arguments) -> begin_match_call (tokenizer, program and input checks) -> route_call (kinds)
//   and the family's own checks (sets) -> lower_programs -> build_tables -> match_fan_out (device cuts, parts, fallback fold) -> match_part per
//   device (buffers, condition hashing, chunked upload, one walker launch per chunk through launch_walker, results back).
// What a family adds to a part is its PartMode (PlanePart: bit planes; WidePart: stored flags, k_eval_row_programs, pair words —
// or, for bsg_match_rows_wide_rows, the same part with the rows policy: three more passes turn the words into tagged row lists on
// the device, headers and payload come back instead, and match_fan_out's finish step stitches the parts into the call's result).
// Which tables a call builds, which walker serves it and what it refuses is host/match_route.hpp's: a CallSpec per entry point,
// route() over the table's kinds, slot() and the list of the 60 walkers (DESIGN.md has the route as a table).  Here: build_tables
// builds what the route says, launch_walker launches the slot's kernel.  The lookup calls are the wide call with another Family and a
// LookupPlan beside its WidePlan (host/lookup_plan.hpp): W flag words per row, match_lookup.hip.h's walker and evaluator.

#include <cassert>
#include <type_traits>

#include "host/match_route.hpp"

namespace {

static_assert(bsh_rxg::kMaxRegexConds == bsg::kRxMaxConds && bsh_rxg::kSingleLdsCap == bsg::kRxLdsCap && bsh_rxg::kManyLdsCap == bsg::kRxManyLdsCap &&
                  bsh_rxg::kSingleSlots == bsg::kRxActive && (bsh_rxg::kManySlots == bsg::kRxManyActive || BSG_RX_MANY_SLOTS != 4) &&
                  bsh_rxg::kPathCap == bsg::kPathCap,
              "host/regex_groups.hpp states the kernels' limits");

// The LDS table blob of a call's FieldRegex conditions (layout: match.hip.h; built by host/regex_groups.hpp).  BSG_E_UNSUPPORTED,
// before anything is launched, for a pattern outside the compiler's subset, more than kRxMaxConds of them, or tables over `cap`
// (kRxLdsCap; kRxManyLdsCap for the batched call, whose blob also holds the conditions' user masks: users [n_conds], else NULL).
// distinct: the regex conditions the blob is built of (the lookup call: each repeated condition once); NULL = every one of the table.
int32_t build_rx_blob(const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                      std::vector<uint32_t> &blob, uint32_t &n_rx, uint32_t cap = bsg::kRxLdsCap, const uint64_t *users = nullptr,
                      const std::vector<uint32_t> *distinct = nullptr)
{
    const bsh_rxg::BlobResult r = distinct ? bsh_rxg::build_blob_of(cond_bytes, cond_off, *distinct, cap, users, blob)
                                           : bsh_rxg::build_blob(cond_bytes, cond_off, cond_kinds, n_conds, BSG_KIND_FIELD_REGEX, cap, users, blob);
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

static_assert(bsh_rxg::kSingleSubLdsCap == bsg::kRxSubLdsCap && bsh_rxg::kManySubLdsCap == bsg::kRxManySubLdsCap,
              "host/regex_groups.hpp states the caps of the regex tables beside a needle table");
static_assert(bsh::kSubWords == bsg::kSubWords && sizeof(uint64_t) * 256 * bsh::kSubWords == bsg::kSubTableBytes && bsh::kSubMaxNeedle == 64,
              "host/substring_pack.hpp states the substring kernels' table");

static_assert(bsh_rxg::kWideSubLdsCap == bsg::kRxWideSubLdsCap, "host/regex_groups.hpp states the cap of the storing walker's regex tables beside a needle table");
static_assert(bsh_wide::kWideLdsCap == bsg::kRxWideLdsCap && sizeof(bsh_wide::EvalItem) == sizeof(bsg::RowEvalItem) &&
                  offsetof(bsh_wide::EvalItem, stride) == offsetof(bsg::RowEvalItem, stride),
              "host/wide_plan.hpp states the kernels' limits and item layout");
static_assert(sizeof(bsh_wide::PairSet) == sizeof(bsg::PairSetDesc) && offsetof(bsh_wide::PairSet, tile0) == offsetof(bsg::PairSetDesc, tile0) &&
                  bsh_wide::kPairScanWidth == bsg::kPairScanWidth && BSG_MATCH_PAIR_SCAN_WIDTH == bsg::kPairScanWidth &&
                  bsh_wide::kPairNone == bsg::kPairNone && bsh_wide::kPairAll == bsg::kPairAll && bsh_wide::kPairList == bsg::kPairList &&
                  bsh_wide::kPairDense == bsg::kPairDense && BSG_ROW_NONE == bsg::kPairNone && BSG_ROW_ALL == bsg::kPairAll &&
                  BSG_ROW_LIST == bsg::kPairList && BSG_ROW_DENSE == bsg::kPairDense,
              "host/wide_plan.hpp and bloomgpu.h state the list passes' set table, scan width and tags");

static_assert(bsh_route::kKindFieldToken == BSG_KIND_FIELD_TOKEN && bsh_route::kKindFieldRegex == BSG_KIND_FIELD_REGEX && bsh_route::kKindSubstring == BSG_KIND_SUBSTRING &&
                  bsh_route::kKindFieldSubstring == BSG_KIND_FIELD_SUBSTRING && bsh_route::kKindFieldRange == BSG_KIND_FIELD_RANGE,
              "host/match_route.hpp states bloomgpu.h's condition kinds");

static_assert(bsh_lookup::kMaxConds == BSG_MATCH_LOOKUP_MAX_CONDS && bsg::lookup_lds_bytes(bsh_lookup::kMaxStringSlots, bsh_lookup::kMaxPairSlots) ==
                                                                      bsg::kMatchLookupLdsBytes,
              "host/lookup_plan.hpp and bloomgpu.h state the lookup walker's limits");

// One row-matcher call.  The entry points fill the caller's arguments; validation and lowering fill the rest.
struct MatchCall {
    const uint8_t *rows;
    const uint64_t *row_off;
    uint32_t n_rows;
    const uint8_t *cond_bytes;             // the condition table: strings 2c (field) and 2c + 1 (token) of condition c
    const uint32_t *cond_off, *cond_kinds;
    uint32_t n_conds;
    uint64_t *out_bits;
    uint32_t *out_fallback_rows;
    uint32_t fallback_cap;
    uint32_t *out_n_fallback;
    uint64_t n_bytes = 0;                  // check_match_inputs
    uint32_t cond_len = 0;
    std::vector<uint32_t> prog;            // lower_programs: the lowered programs behind each other
    std::vector<uint32_t> prog_off{0};     // [n_queries + 1] into prog
    std::vector<uint32_t> rx_blob;         // build_rx_blob
    uint32_t n_rx = 0;
    bool substr = false;                   // build_sub_tables: the call holds the substring walkers' tables
    bsh::NeedlePack sub;                   // ... M, START, ANY
    std::vector<uint32_t> sub_kinds;       // ... and cond_kinds with word | end bit of a substring condition's needle (match.hip.h SubLane)
    bool range = false;                    // build_range_table: the table holds a FieldRange condition
    std::vector<uint32_t> range_conds;     // ... the conditions of kind 6,
    std::vector<uint64_t> range_bounds;    // ... lo and hi of each (two's complement), in that order
    std::vector<uint32_t> range_kinds;     // ... and cond_kinds with a range condition's flags << 8 (match.hip.h NumLane)
    bsg::TokSpec spec{};                   // tok_spec
    bool default_tok = true;
    const bsh_route::CallSpec *call = nullptr;   // the entry point (route_call)
    bsh_route::Route route;                // ... and what its table asks for: the tables to build, the walker's consumers, the name in traces
    uint32_t slot = bsh_route::kNoSlot;    // ... and the walker: bsh_route::slot of the call's mode, those consumers and the tokenizer
    bool three() const { return route.consumers == bsh_route::Consumers::RegexSubstrRange; }
    bool need_bits() const { return call->policy != bsh_route::Policy::Hist; }   // (bsg_match_rows_wide_hist's result is its counters: out_bits is NULL and never read)
};

// What differs between the families in the shared checks: limits and the words their messages name the call by.
struct Family {
    uint32_t max_queries;
    const char *call;                      // "%u queries (one <call> match call holds %u)"
    uint32_t max_ops;
    const char *programs_of;               // "the <programs_of> programs hold more than ..."; NULL: the single call's one message
    uint32_t max_conds = bsg::kMatchMaxConds;
};
constexpr Family kSingleFamily{1, "single", bsg::kMatchMaxOps, nullptr};
constexpr Family kManyFamily{bsg::kMatchManyMaxQueries, "batched", bsg::kMatchManyMaxOps, "batch's"};
constexpr Family kWideFamily{bsh_wide::kMaxQueries, "wide", bsh_wide::kMaxOps, "call's"};
constexpr Family kLookupFamily{bsh_wide::kMaxQueries, "lookup", bsh_wide::kMaxOps, "call's", bsh_lookup::kMaxConds};
constexpr Family kLookupRegexFamily{bsh_wide::kMaxQueries, "lookup regex", bsh_wide::kMaxOps, "call's", bsh_lookup::kMaxConds};

// What every row-matcher call checks of its rows and conditions (the kinds themselves are the caller's); cond_len / n_bytes out.
int32_t check_match_inputs(const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows, const uint8_t *cond_bytes, const uint32_t *cond_off,
                           const uint32_t *cond_kinds, uint32_t n_conds, const uint64_t *out_bits, const uint32_t *out_n_fallback,
                           uint32_t &cond_len, uint64_t &n_bytes, uint32_t max_conds = bsg::kMatchMaxConds, bool need_bits = true)
{
    if (!out_n_fallback || (n_rows && (!row_off || (need_bits && !out_bits)))) return fail(BSG_E_INVALID, "null argument");
    if (n_conds && (!cond_off || !cond_kinds)) return fail(BSG_E_INVALID, "conditions are null");
    if (n_conds > max_conds) return fail(BSG_E_UNSUPPORTED, "%u conditions (the device matcher holds %u)", n_conds, max_conds);
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

// The head of every call: the tokenizer spec, the query limit, the program table and check_match_inputs.
int32_t begin_match_call(MatchCall &mc, const bsh_route::CallSpec &call, const Family &f, const bsg_tokenizer *tok_in, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries)
{
    bsg_tokenizer rec{};
    mc.call = &call;
    if (int32_t rc = tok_spec(tok_in, rec, mc.spec, mc.default_tok)) return rc;
    if (n_queries > f.max_queries) return fail(BSG_E_UNSUPPORTED, "%u queries (one %s match call holds %u)", n_queries, f.call, f.max_queries);
    if (n_queries && !prog_off) return fail(BSG_E_INVALID, "prog_off is null");
    for (uint32_t q = 0; q < n_queries; ++q)
        if (prog_off[q + 1] < prog_off[q]) return fail(BSG_E_INVALID, "prog_off not monotone at %u", q);
    if (n_queries && prog_off[n_queries] > prog_off[0] && !prog_ops) return fail(BSG_E_INVALID, "prog_ops is null");
    return check_match_inputs(mc.rows, mc.row_off, mc.n_rows, mc.cond_bytes, mc.cond_off, mc.cond_kinds, mc.n_conds, mc.out_bits, mc.out_n_fallback,
                              mc.cond_len, mc.n_bytes, f.max_conds, mc.need_bits());
}

// Every query's program lowered over the identity term positions (the lookup call: over term_pos, where a repeated condition is its
// first occurrence) into mc.prog / mc.prog_off: depth <= 64 per query, f.max_ops in all.
int32_t lower_programs(MatchCall &mc, const Family &f, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                       const std::vector<uint32_t> *term_pos = nullptr)
{
    std::vector<uint32_t> ident(mc.n_conds), one;
    for (uint32_t c = 0; c < mc.n_conds; ++c) ident[c] = term_pos ? (*term_pos)[c] : c;
    for (uint32_t q = 0; q < n_queries; ++q) {
        uint32_t depth = 1;
        if (int32_t rc = lower_program(prog_ops + prog_off[q], prog_off[q + 1] - prog_off[q], mc.n_conds, ident, one, depth)) return rc;
        if (!f.programs_of) {
            if (depth > 64 || one.size() > f.max_ops)
                return fail(BSG_E_UNSUPPORTED, "expression too large for the device matcher (depth %u, %zu ops)", depth, one.size());
        } else if (depth > 64) {
            return fail(BSG_E_UNSUPPORTED, "query %u: expression too deep for the device matcher (depth %u)", q, depth);
        }
        mc.prog.insert(mc.prog.end(), one.begin(), one.end());
        if (mc.prog.size() > f.max_ops)
            return fail(BSG_E_UNSUPPORTED, "the %s programs hold more than %u lowered ops (at query %u)", f.programs_of, f.max_ops, q);
        mc.prog_off.push_back((uint32_t)mc.prog.size());
    }
    return BSG_OK;
}

// The needle tables of a call's Substring / FieldSubstring conditions: each needle (entry 2c + 1, raw) is checked and folded under
// the call's own tokenizer, then all are packed first-fit.  BSG_E_INVALID for an empty needle or invalid UTF-8, BSG_E_UNSUPPORTED
// for a needle over 64 folded bytes or needles that do not fit the kSubWords x 64 positions, before anything is launched.
// mc.cond_kinds then points at the kinds with each needle's place.
int32_t build_sub_tables(MatchCall &mc)
{
    bsh::Tokenizer t;                      // only lower() is read: separators and the width play no part in the exact test
    if (!mc.default_tok) t.flags = mc.spec.flags;
    std::vector<std::string> folded;
    std::vector<uint8_t> any_field;
    std::vector<uint32_t> cond_of;
    for (uint32_t c = 0; c < mc.n_conds; ++c) {
        if (mc.cond_kinds[c] != BSG_KIND_SUBSTRING && mc.cond_kinds[c] != BSG_KIND_FIELD_SUBSTRING) continue;
        const std::string_view needle((const char *)mc.cond_bytes + mc.cond_off[2 * c + 1], mc.cond_off[2 * c + 2] - mc.cond_off[2 * c + 1]);
        folded.emplace_back();
        switch (bsh::fold_needle(needle, t, folded.back())) {
        case bsh::NeedleStatus::Ok: break;
        case bsh::NeedleStatus::Invalid: return fail(BSG_E_INVALID, "condition %u: a needle is non-empty valid UTF-8", c);
        default: return fail(BSG_E_UNSUPPORTED, "condition %u: a needle of %zu bytes after folding (the device matcher holds %u)", c, folded.back().size(), bsh::kSubMaxNeedle);
        }
        any_field.push_back(mc.cond_kinds[c] == BSG_KIND_SUBSTRING);
        cond_of.push_back(c);
    }
    if (!bsh::pack_needles(folded, any_field, mc.sub))
        return fail(BSG_E_UNSUPPORTED, "the needles of %zu substring conditions do not fit %u words of 64 bytes", folded.size(), bsh::kSubWords);
    mc.sub_kinds.assign(mc.cond_kinds, mc.cond_kinds + mc.n_conds);
    for (size_t i = 0; i < cond_of.size(); ++i) mc.sub_kinds[cond_of[i]] |= mc.sub.where[i] << 8;   // word << 8 | end bit << 16
    mc.cond_kinds = mc.sub_kinds.data();
    mc.substr = true;
    return BSG_OK;
}

// The bounds of a call's FieldRange conditions: entry 2c + 1 is lo (int64, little-endian), hi (the same) and one flag byte
// (BSG_RANGE_*).  BSG_E_INVALID, naming the condition, for another length or a flag bit above 3.  A table without a kind-6 condition
// leaves the call as it is; else mc.cond_kinds then points at the kinds with each condition's flags.
int32_t build_range_table(MatchCall &mc)
{
    for (uint32_t c = 0; c < mc.n_conds; ++c) {
        if (mc.cond_kinds[c] != BSG_KIND_FIELD_RANGE) continue;
        const uint32_t at = mc.cond_off[2 * c + 1], len = mc.cond_off[2 * c + 2] - at;
        if (len != BSG_RANGE_ENTRY_BYTES) return fail(BSG_E_INVALID, "condition %u: a range entry is %u bytes (lo, hi, flags), not %u", c, BSG_RANGE_ENTRY_BYTES, len);
        const uint8_t *b = mc.cond_bytes + at;
        if (b[16] > 15u) return fail(BSG_E_INVALID, "condition %u: range flags 0x%02x (bits 0-3 are defined)", c, b[16]);
        uint64_t lo = 0, hi = 0;
        for (uint32_t i = 0; i < 8; ++i) { lo |= (uint64_t)b[i] << (8 * i); hi |= (uint64_t)b[8 + i] << (8 * i); }
        if (!mc.range) mc.range_kinds.assign(mc.cond_kinds, mc.cond_kinds + mc.n_conds);
        mc.range = true;
        mc.range_kinds[c] |= (uint32_t)b[16] << 8;
        mc.range_conds.push_back(c);
        mc.range_bounds.push_back(lo);
        mc.range_bounds.push_back(hi);
    }
    if (mc.range) mc.cond_kinds = mc.range_kinds.data();
    return BSG_OK;
}
static_assert(BSG_RANGE_NO_LO == bsg::kRangeNoLo && BSG_RANGE_NO_HI == bsg::kRangeNoHi && BSG_RANGE_LO_OPEN == bsg::kRangeLoOpen &&
                  BSG_RANGE_HI_OPEN == bsg::kRangeHiOpen && BSG_KIND_FIELD_RANGE == 6u,
              "bloomgpu.h states the range walkers' kind and flags");

// ---- the sixty walkers: (single / many / wide / lookup) x (consumer set) x (default tokenizer / spec / spec with an n-gram width) ----
// What a launch may hand a walker; each kernel takes the members its own parameter list names, in its own order.
struct LaunchArgs {
    hipStream_t stream;
    hipEvent_t k0, k1;                     // one chunk's walk lies between them
    bsg::MatchArgs a;                      // a.n_rows rows, one per lane
    bsg::RxArgs rx;
    bsg::SubArgs sub;
    bsg::TokSpec tok;
    bsg::MatchManyArgs many{};             // the mode's own argument struct (the single call has none)
    bsg::MatchWideArgs wide{};
    bsg::MatchLookupArgs lookup{};
    template <class T>
    const T &get() const
    {
        if constexpr (std::is_same_v<T, bsg::MatchArgs>) return a;
        else if constexpr (std::is_same_v<T, bsg::RxArgs>) return rx;
        else if constexpr (std::is_same_v<T, bsg::SubArgs>) return sub;
        else if constexpr (std::is_same_v<T, bsg::TokSpec>) return tok;
        else if constexpr (std::is_same_v<T, bsg::MatchManyArgs>) return many;
        else if constexpr (std::is_same_v<T, bsg::MatchWideArgs>) return wide;
        else { static_assert(std::is_same_v<T, bsg::MatchLookupArgs>, "a walker parameter LaunchArgs does not hold"); return lookup; }
    }
};
template <class... P>
void launch_as(void (*k)(P...), uint32_t lds, const LaunchArgs &l)
{
    const dim3 grid((l.a.n_rows + bsg::kIngestThreads - 1) / bsg::kIngestThreads), block(bsg::kIngestThreads);
    hipExtLaunchKernelGGL(k, grid, block, lds, l.stream, l.k0, l.k1, 0, l.get<P>()...);
}
template <auto K>
void launch_thunk(uint32_t lds, const LaunchArgs &l) { launch_as(K, lds, l); }

// a slot's kernel takes RxArgs iff its consumers hold regex, SubArgs iff they hold substr, the mode's struct and no other mode's,
// TokSpec iff the tokenizer is a spec
template <class K> struct WalkerParams;
template <class... P>
struct WalkerParams<void (*)(P...)> {
    template <class T> static constexpr bool takes = (std::is_same_v<T, P> || ...);
    static constexpr bool fits(bsh_route::Mode m, bsh_route::Consumers c, bsh_route::Tok t)
    {
        return takes<bsg::MatchArgs> && takes<bsg::RxArgs> == bsh_route::has_regex(c) && takes<bsg::SubArgs> == bsh_route::has_substr(c) &&
               takes<bsg::MatchManyArgs> == (m == bsh_route::Mode::Many) && takes<bsg::MatchWideArgs> == (m == bsh_route::Mode::Wide) &&
               takes<bsg::MatchLookupArgs> == (m == bsh_route::Mode::Lookup) && takes<bsg::TokSpec> == (t != bsh_route::Tok::Default);
    }
};
#define BSG_WALKER_FITS(M, C, T, K) \
    static_assert(WalkerParams<decltype(&bsg::K)>::fits(bsh_route::Mode::M, bsh_route::Consumers::C, bsh_route::Tok::T), #K " does not take what its slot says");
BSH_MATCH_WALKERS(BSG_WALKER_FITS)
#undef BSG_WALKER_FITS

using WalkerLaunch = void (*)(uint32_t lds, const LaunchArgs &);
struct WalkerTable { WalkerLaunch at[bsh_route::kSlots]; };
constexpr WalkerTable walker_table()
{
    WalkerTable t{};
#define BSG_WALKER_SLOT(M, C, T, K) t.at[bsh_route::slot(bsh_route::Mode::M, bsh_route::Consumers::C, bsh_route::Tok::T)] = &launch_thunk<&bsg::K>;
    BSH_MATCH_WALKERS(BSG_WALKER_SLOT)
#undef BSG_WALKER_SLOT
    return t;
}
constexpr WalkerTable kWalkers = walker_table();

// the bytes of a blob cap the route names
constexpr uint32_t cap_bytes(bsh_route::Cap c)
{
    switch (c) {
    case bsh_route::Cap::Single: return bsh_rxg::kSingleLdsCap;
    case bsh_route::Cap::SingleSub: return bsh_rxg::kSingleSubLdsCap;
    case bsh_route::Cap::Many: return bsh_rxg::kManyLdsCap;
    case bsh_route::Cap::ManySub: return bsh_rxg::kManySubLdsCap;
    case bsh_route::Cap::Wide: return bsh_wide::kWideLdsCap;
    case bsh_route::Cap::WideSub: return bsh_rxg::kWideSubLdsCap;
    default: return 0;                     // None: no blob; Lookup: build_tables asks the call's own plan
    }
}

// Dynamic LDS of a slot's launch: this base plus the regex blob's bytes (a call without regex conditions has no blob).  The substring
// consumer adds its needle table; the lookup walkers' base is what the launch's own tables take.
constexpr uint32_t walker_lds_base(bsh_route::Mode m, bsh_route::Consumers c)
{
    const bool sub = bsh_route::has_substr(c);
    switch (m) {
    case bsh_route::Mode::Single: return sub ? bsg::kMatchSubLdsBytes : bsg::kMatchLdsBytes;
    case bsh_route::Mode::Many: return sub ? bsg::kMatchManySubLdsBytes : bsg::kMatchManyLdsBytes;
    case bsh_route::Mode::Wide: return sub ? bsg::kMatchWideSubLdsBytes : bsg::kMatchWideLdsBytes;
    default: return 0;
    }
}

// one chunk's walk by the call's walker (mc.slot)
void launch_walker(const MatchCall &mc, const LaunchArgs &l)
{
    const bsh_route::Mode m = mc.call->mode;
    const bsh_route::Consumers c = mc.route.consumers;
    const uint32_t base = m == bsh_route::Mode::Lookup ? bsg::lookup_lds_bytes(l.lookup.n_str_slots, l.lookup.n_pair_slots) : walker_lds_base(m, c);
    // a call that takes no regex walker refuses FieldRegex conditions before it gets here; the blob was built under the route's cap
    // (the lookup call: under what this table's LDS leaves)
    assert(mc.slot < bsh_route::kSlots && kWalkers.at[mc.slot] && (!l.rx.n_rx || bsh_route::has_regex(c)) && (!bsh_route::has_substr(c) || l.sub.table));
    assert(m == bsh_route::Mode::Lookup ? base + l.rx.n_words * 4 <= bsh_lookup::kWorkgroupLds : l.rx.n_words * 4 <= cap_bytes(mc.route.cap));
    assert(!mc.three() || (mc.substr && mc.range));
    kWalkers.at[mc.slot](base + l.rx.n_words * 4, l);
}

// ---- one part: rows [r0, r1) of a call on one device ----
// What match_part hands a mode's hooks: the device (its lock held), the part's scratch and what is on the device already.
struct PartDev {
    Device &d;
    Scratch &scratch;
    uint32_t r0, n_rows;
    uint32_t *d_prog = nullptr, *d_poff = nullptr;     // the call's lowered programs and (mode.prog_off()) their offsets
    bsg::RxArgs rx{};                                  // the regex blob
    bsg::SubArgs sub{};                                // the needle tables (mc.substr)
    const uint64_t *d_ch = nullptr;                    // [2 * n_conds][4]: the condition strings' base hashes (k_hash_fp_entries, enqueued)
};

// bsg_match_rows_many: what a part needs beyond the call.  mc.prog then holds the lowered programs of all queries behind each other
// and out_bits n_queries planes of call_words words.
struct ManyPlan {
    const uint32_t *set_first_row;         // the call's set table (n_sets == 0: every query on every row)
    const uint64_t *set_mask;
    uint32_t n_sets, n_queries;
    size_t call_words;
};

// The single and the batched calls: the walker evaluates, one plane of bits per query.  r0 is a multiple of 64: whole words.
struct PlanePart {
    static constexpr const char *kPlanned = "offsets rebased, lock taken", *kBack = "matched, bits back";
    const MatchCall &mc;
    const ManyPlan *many;                              // NULL = one expression
    bsh_wide::SetRange sets;                           // the part's sets, their first rows counted from r0
    uint32_t n_sets = 0;
    size_t n_words = 0, n_planes = 1;
    uint64_t *d_bits = nullptr, *d_smask = nullptr;
    uint32_t *d_sfirst = nullptr;

    const char *tag() const { return mc.route.trace; }
    bool prog_off() const { return many != nullptr; }
    int32_t plan(uint32_t r0, uint32_t r1)
    {
        n_words = ((size_t)(r1 - r0) + 63) / 64;
        if (many) n_planes = many->n_queries;
        if (many && many->n_sets) {
            sets = bsh_wide::part_set_range(many->set_first_row, many->n_sets, r0, r1);
            n_sets = sets.n();
        }
        return BSG_OK;
    }
    int32_t alloc(PartDev &p)
    {
        HIP_TRY(p.scratch.alloc(&d_bits, n_words * n_planes * 8));
        if (n_sets) {
            HIP_TRY(p.scratch.alloc(&d_sfirst, ((size_t)n_sets + 1) * 4));
            HIP_TRY(p.scratch.alloc(&d_smask, (size_t)n_sets * 8));
        }
        return BSG_OK;
    }
    int32_t upload(PartDev &p)
    {
        if (n_sets) {
            HIP_TRY(hipMemcpyAsync(d_sfirst, sets.first_row.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, p.d.stream));
            HIP_TRY(hipMemcpyAsync(d_smask, many->set_mask + sets.s0, (size_t)n_sets * 8, hipMemcpyHostToDevice, p.d.stream));
        }
        return BSG_OK;
    }
    void launch(PartDev &p, bsg::MatchArgs &a, uint32_t rf, hipEvent_t k0, hipEvent_t k1)
    {
        a.prog = p.d_prog; a.n_ops = (uint32_t)mc.prog.size(); a.out_bits = d_bits + rf / 64;
        LaunchArgs l{p.d.stream, k0, k1, a, p.rx, p.sub, mc.spec};
        if (many) l.many = bsg::MatchManyArgs{p.d_poff, d_sfirst, d_smask, n_words, many->n_queries, n_sets};
        launch_walker(mc, l);
    }
    int32_t results(PartDev &p, EventList &)           // this part's words of every plane
    {
        if (!many || many->call_words == n_words)
            HIP_TRY(hipMemcpyAsync(mc.out_bits + p.r0 / 64, d_bits, n_words * n_planes * 8, hipMemcpyDeviceToHost, p.d.stream));
        else
            HIP_TRY(hipMemcpy2DAsync(mc.out_bits + p.r0 / 64, many->call_words * 8, d_bits, n_words * 8, n_words * 8, n_planes, hipMemcpyDeviceToHost, p.d.stream));
        return BSG_OK;
    }
    void landed() {}
    void more_fallback(std::vector<uint32_t> &) {}
};

// bsg_match_rows_wide_rows: where the call's tagged row lists go
struct WideRowsOut {
    uint32_t *hdr;                             // [n_pairs]
    uint64_t *off;                             // [n_pairs + 1] or NULL
    uint32_t *payload;
    uint64_t cap, *len;
};
// bsg_match_rows_wide_hist: the bucket rule and where the call's counts go
struct WideHistOut {
    bsg::HistField field;
    int64_t origin;
    uint64_t width;
    uint32_t n_buckets;
    uint32_t *counts;                          // [n_pairs * BSG_HIST_SLOTS(n_buckets)]
    uint32_t slots() const { return BSG_HIST_SLOTS(n_buckets); }
};
// bsg_match_rows_wide: what a part needs beyond the call (sets always materialised: the implicit set is one set with every query)
struct WidePlan {
    const uint32_t *set_first_row, *set_query_off, *set_queries;
    uint32_t n_sets, n_queries;
    std::vector<uint64_t> set_cond_mask;       // [n_sets]
    std::vector<uint32_t> set_rx_mask;         // [n_sets] bsg_match_rows_lookup_regex(_rows): the regex slots the set's queries use
    std::vector<uint64_t> set_word0;           // [n_sets + 1]: the first result word of the set's first pair
    const WideRowsOut *rows = nullptr;         // the rows policy: lists instead of words
    const bsh_lookup::Plan *lookup = nullptr;  // bsg_match_rows_lookup(_rows) / _lookup_regex(_rows): the table's strings, roles and pairs
    const WideHistOut *hist = nullptr;         // the hist policy: bucketed counts instead of words
};

// The wide call: the storing walk chunk by chunk, then one evaluation launch over the part's items (r0 a set-relative multiple of 64).
// direct: the part is the whole call and its words go straight to out_bits; else they are scattered on the host into the call's
// layout (a set cut by a part boundary has some of its tiles here and some on the next device).
struct WidePart {
    static constexpr const char *kPlanned = "part planned, lock taken", *kBack = "matched, words back";
    const MatchCall &mc;
    const WidePlan &wp;
    const bool direct;
    bsh_wide::PartSets ps;
    uint32_t n_sets = 0, pair0 = 0, n_pairs = 0;
    std::vector<uint32_t> pair_off_local;
    std::vector<bsh_wide::EvalItem> items;
    uint64_t part_words = 0;
    std::vector<uint64_t> staged;
    uint8_t *d_state = nullptr;
    uint64_t *d_sat = nullptr, *d_out = nullptr, *d_smask = nullptr;
    uint32_t *d_sfirst = nullptr, *d_spair = nullptr, *d_pairs = nullptr;
    bsg::RowEvalItem *d_items = nullptr;
    // the rows policy: the words stay on the device, k_pair_sizes / k_pair_scan_* / k_pair_write make the lists, headers and
    // payload_len u32 of payload come back (direct: into the caller's buffers, when the payload fits; else staged for the stitch)
    std::vector<bsh_wide::PairSet> psets;
    std::vector<uint32_t> staged_hdr, staged_payload;
    uint64_t payload_len = 0;
    bsg::PairSetDesc *d_psets = nullptr;
    uint32_t *d_phdr = nullptr, *d_payload = nullptr;
    uint64_t *d_psize = nullptr, *d_poffs = nullptr, *d_bsum = nullptr;
    // the lookup family: W flag words per row (word-major over the part's rows), the tables placed from the device's hashes
    uint32_t flag_words = 1;
    std::vector<uint64_t> cond_h, str_h0, pair_tab;
    std::vector<uint32_t> str_tab;
    uint32_t *d_lk_str = nullptr, *d_lk_rxmask = nullptr;
    uint64_t *d_lk_pair = nullptr, *d_lk_rec = nullptr;
    // the hist policy: k_bucket_rows beside every chunk's walk leaves a u16 code per row, k_pair_hist folds the words and the codes
    // into n_pairs * slots counters; those come back (direct: into the caller's array; else staged, added by the finish step) with
    // the scanner's own list of undecided rows
    uint16_t *d_code = nullptr;
    uint32_t *d_counts = nullptr, *d_hfb = nullptr, *d_nhfb = nullptr;
    EventList hev;                                     // the scanner's launches and k_pair_hist: start, stop each
    std::vector<uint32_t> staged_counts, hist_fb;
    float hist_ms = 0.f;
    int hist_dev = 0;                                  // the device the part ran on (bsg_last_hist_ms: per device the sum of its parts)
    hipError_t hist_err = hipSuccess;                  // what a scanner launch met (launch() returns nothing)

    const char *tag() const { return mc.route.trace; }
    bool prog_off() const { return true; }
    int32_t plan(uint32_t r0, uint32_t r1)
    {
        ps = bsh_wide::part_sets(wp.set_first_row, wp.set_query_off, wp.n_sets, r0, r1);
        n_sets = ps.n(); pair0 = ps.pair_off[0]; n_pairs = ps.pair_off[n_sets] - pair0;
        pair_off_local = ps.pair_off;
        for (uint32_t &v : pair_off_local) v -= pair0;
        if (!bsh_wide::eval_items(ps, items, part_words))
            return fail(BSG_E_UNSUPPORTED, "more than %u (tile, pair range) items on one device", bsh_wide::kMaxItems);
        if (wp.rows || wp.hist) psets = bsh_wide::pair_sets(ps);
        return BSG_OK;
    }
    int32_t alloc(PartDev &p)
    {
        if (wp.lookup) {
            flag_words = bsh_lookup::flag_words(mc.n_conds);
            HIP_TRY(p.scratch.alloc(&d_lk_str, (size_t)bsh_lookup::table_slots(wp.lookup->n_strings()) * 4));
            HIP_TRY(p.scratch.alloc(&d_lk_pair, (size_t)bsh_lookup::table_slots((uint32_t)wp.lookup->pairs.size()) * 8));
            HIP_TRY(p.scratch.alloc(&d_lk_rec, std::max<size_t>(wp.lookup->n_strings(), 1) * 8));
        }
        HIP_TRY(p.scratch.alloc(&d_sat, (size_t)p.n_rows * 8 * flag_words));
        HIP_TRY(p.scratch.alloc(&d_state, (size_t)p.n_rows));
        HIP_TRY(p.scratch.alloc(&d_out, std::max<uint64_t>(part_words, 1) * 8));
        HIP_TRY(p.scratch.alloc(&d_sfirst, ((size_t)n_sets + 1) * 4));
        HIP_TRY(p.scratch.alloc(&d_spair, ((size_t)n_sets + 1) * 4));
        if (mc.n_rx && wp.lookup) HIP_TRY(p.scratch.alloc(&d_lk_rxmask, (size_t)n_sets * 4));     // the lookup walker reads no condition mask
        else HIP_TRY(p.scratch.alloc(&d_smask, (size_t)n_sets * 8));
        HIP_TRY(p.scratch.alloc(&d_pairs, std::max<size_t>(n_pairs, 1) * 4));
        HIP_TRY(p.scratch.alloc(&d_items, std::max<size_t>(items.size(), 1) * sizeof(bsg::RowEvalItem)));
        if (wp.rows && n_pairs) {
            HIP_TRY(p.scratch.alloc(&d_psets, psets.size() * sizeof(bsg::PairSetDesc)));
            HIP_TRY(p.scratch.alloc(&d_phdr, (size_t)n_pairs * 4));
            HIP_TRY(p.scratch.alloc(&d_psize, (size_t)n_pairs * 8));
            HIP_TRY(p.scratch.alloc(&d_poffs, ((size_t)n_pairs + 1) * 8));
            HIP_TRY(p.scratch.alloc(&d_bsum, (size_t)scan_blocks() * 8));
            HIP_TRY(p.scratch.alloc(&d_payload, std::max<uint64_t>(part_words, 1) * 8));      // the bound: 2 u32 per word
        }
        if (wp.hist) {
            HIP_TRY(p.scratch.alloc(&d_code, std::max<size_t>(p.n_rows, 1) * 2));
            HIP_TRY(p.scratch.alloc(&d_counts, std::max<size_t>((size_t)n_pairs * wp.hist->slots(), 1) * 4));
            HIP_TRY(p.scratch.alloc(&d_hfb, std::max<size_t>(p.n_rows, 1) * 4));
            HIP_TRY(p.scratch.alloc(&d_nhfb, 4));
            if (n_pairs) HIP_TRY(p.scratch.alloc(&d_psets, psets.size() * sizeof(bsg::PairSetDesc)));
        }
        return BSG_OK;
    }
    uint32_t scan_blocks() const { return (n_pairs + bsg::kPairScanWidth - 1) / bsg::kPairScanWidth; }
    int32_t upload(PartDev &p)
    {
        HIP_TRY(hipMemcpyAsync(d_sfirst, ps.first_row.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, p.d.stream));
        HIP_TRY(hipMemcpyAsync(d_spair, pair_off_local.data(), ((size_t)n_sets + 1) * 4, hipMemcpyHostToDevice, p.d.stream));
        if (d_lk_rxmask) HIP_TRY(hipMemcpyAsync(d_lk_rxmask, wp.set_rx_mask.data() + ps.s0, (size_t)n_sets * 4, hipMemcpyHostToDevice, p.d.stream));
        else HIP_TRY(hipMemcpyAsync(d_smask, wp.set_cond_mask.data() + ps.s0, (size_t)n_sets * 8, hipMemcpyHostToDevice, p.d.stream));
        if (n_pairs) HIP_TRY(hipMemcpyAsync(d_pairs, wp.set_queries + pair0, (size_t)n_pairs * 4, hipMemcpyHostToDevice, p.d.stream));
        if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(bsg::RowEvalItem), hipMemcpyHostToDevice, p.d.stream));
        if (d_psets) HIP_TRY(hipMemcpyAsync(d_psets, psets.data(), psets.size() * sizeof(bsg::PairSetDesc), hipMemcpyHostToDevice, p.d.stream));
        if (wp.hist) HIP_TRY(hipMemsetAsync(d_nhfb, 0, 4, p.d.stream));
        if (wp.lookup) return upload_lookup(p);
        return BSG_OK;
    }
    // The bucket scanner over one chunk's rows [rf, rf + n), beside the chunk's walk: a contiguous run of rows per wave, as the
    // MinMax scanner.  One set with a pair (the implicit set, or a part inside one set): no set search.
    void launch_scanner(PartDev &p, const bsg::MatchArgs &a, uint32_t rf)
    {
        if (!a.n_rows || !n_pairs) return;             // (a part without a pair: nothing is walked, nothing is counted)
        const size_t k = hev.v.size();
        if (hipError_t e = hev.add(2); e != hipSuccess) { hist_err = e; return; }
        const WideHistOut &ho = *wp.hist;
        bsg::BucketArgs b{};
        b.rows = a.rows; b.row_off = a.row_off - rf;
        b.set_first_row = d_sfirst; b.set_pair_off = d_spair;
        b.code = d_code; b.fallback_rows = d_hfb; b.n_fallback = d_nhfb;
        b.origin = ho.origin; b.width = ho.width; b.n_buckets = ho.n_buckets; b.n_sets = n_sets;
        b.row_first = rf; b.row_end = rf + a.n_rows;
        const bsh::WaveRuns runs = bsh::wave_runs(a.n_rows, p.d.n_cus, 8, bsg::kBucketThreads);
        b.rows_per_wave = runs.rows_per_wave;
        const dim3 grid(runs.grid), block(bsg::kBucketThreads);
        if (n_sets == 1) hipExtLaunchKernelGGL(bsg::k_bucket_rows, grid, block, 0, p.d.stream, hev.v[k], hev.v[k + 1], 0, b, ho.field);
        else hipExtLaunchKernelGGL(bsg::k_bucket_rows_sets, grid, block, 0, p.d.stream, hev.v[k], hev.v[k + 1], 0, b, ho.field);
    }
    // The lookup tables: word 0 of every role string's base hash comes back from the device (the strings are hashed there, under the
    // context's key, like every family's), the host places the slots, tables and role records go up; the flags start at zero.
    int32_t upload_lookup(PartDev &p)
    {
        const bsh_lookup::Plan &pl = *wp.lookup;
        const uint32_t n = pl.n_strings();
        if (n) {
            cond_h.resize((size_t)mc.n_conds * 2 * 4);
            HIP_TRY(hipMemcpyAsync(cond_h.data(), p.d_ch, cond_h.size() * 8, hipMemcpyDeviceToHost, p.d.stream));
            HIP_TRY(hipStreamSynchronize(p.d.stream));
        }
        str_h0.resize(n);
        for (uint32_t id = 0; id < n; ++id) str_h0[id] = cond_h[(size_t)bsh_lookup::rec_entry(pl.rec[id]) * 4];
        str_tab = bsh_lookup::place_strings(str_h0.data(), n);
        pair_tab = bsh_lookup::place_pairs(pl.pairs);
        HIP_TRY(hipMemcpyAsync(d_lk_str, str_tab.data(), str_tab.size() * 4, hipMemcpyHostToDevice, p.d.stream));
        HIP_TRY(hipMemcpyAsync(d_lk_pair, pair_tab.data(), pair_tab.size() * 8, hipMemcpyHostToDevice, p.d.stream));
        if (n) HIP_TRY(hipMemcpyAsync(d_lk_rec, pl.rec.data(), (size_t)n * 8, hipMemcpyHostToDevice, p.d.stream));
        HIP_TRY(hipMemsetAsync(d_sat, 0, (size_t)p.n_rows * 8 * flag_words, p.d.stream));
        return BSG_OK;
    }
    void launch(PartDev &p, bsg::MatchArgs &a, uint32_t rf, hipEvent_t k0, hipEvent_t k1)
    {
        if (wp.hist) launch_scanner(p, a, rf);
        LaunchArgs l{p.d.stream, k0, k1, a, p.rx, p.sub, mc.spec};
        if (wp.lookup)
            l.lookup = bsg::MatchLookupArgs{d_sfirst, d_spair, d_lk_str, d_lk_pair, d_lk_rec, d_sat + rf, d_state + rf, n_sets, (uint32_t)str_tab.size(),
                                            (uint32_t)pair_tab.size(), p.n_rows, bsh_lookup::pair_shift((uint32_t)pair_tab.size()), d_lk_rxmask};
        else l.wide = bsg::MatchWideArgs{d_sfirst, d_smask, d_spair, d_sat + rf, d_state + rf, n_sets};
        launch_walker(mc, l);
    }
    int32_t results(PartDev &p, EventList &kev)        // the evaluation between two more events, then the part's words
    {
        if (!items.empty()) {
            const size_t k = kev.v.size();
            HIP_TRY(kev.add(2));
            const bsg::RowEvalArgs e{d_items, d_pairs, p.d_poff, p.d_prog, d_sat, d_state, d_out, (uint32_t)items.size()};
            const uint32_t per_block = bsg::kRowEvalThreads / 64;
            const dim3 grid(((uint32_t)items.size() + per_block - 1) / per_block), block(bsg::kRowEvalThreads);
            if (wp.lookup) hipExtLaunchKernelGGL(bsg::k_eval_row_programs_w, grid, block, 0, p.d.stream, kev.v[k], kev.v[k + 1], 0, bsg::RowEvalWArgs{e, p.n_rows});
            else hipExtLaunchKernelGGL(bsg::k_eval_row_programs, grid, block, 0, p.d.stream, kev.v[k], kev.v[k + 1], 0, e);
            HIP_TRY(hipGetLastError());
        }
        if (wp.rows) return rows_results(p, kev);
        if (wp.hist) return hist_results(p);
        if (part_words) {
            uint64_t *dst = mc.out_bits + wp.set_word0[ps.s0];
            if (!direct) { staged.resize(part_words); dst = staged.data(); }
            HIP_TRY(hipMemcpyAsync(dst, d_out, part_words * 8, hipMemcpyDeviceToHost, p.d.stream));
        }
        return BSG_OK;
    }
    // The list passes between two more events (the first kernel's start, the last one's stop), then the headers, the payload's
    // length (the stream is waited for: it sizes the copy) and that much payload.
    int32_t rows_results(PartDev &p, EventList &kev)
    {
        if (!n_pairs) return BSG_OK;
        const size_t k = kev.v.size();
        HIP_TRY(kev.add(2));
        const bsg::PairRowsArgs a{d_psets, d_out, d_phdr, d_psize, d_poffs, d_bsum, d_payload, n_pairs, n_sets};
        const dim3 waves((n_pairs + bsg::kPairThreads / 64 - 1) / (bsg::kPairThreads / 64)), scan(scan_blocks());
        hipExtLaunchKernelGGL(bsg::k_pair_sizes, waves, dim3(bsg::kPairThreads), 0, p.d.stream, kev.v[k], nullptr, 0, a);
        hipLaunchKernelGGL(bsg::k_pair_scan_sums, scan, dim3(bsg::kPairScanWidth), 0, p.d.stream, a);
        hipLaunchKernelGGL(bsg::k_pair_scan_blocks, dim3(1), dim3(bsg::kPairScanWidth), 0, p.d.stream, a, scan_blocks());
        hipLaunchKernelGGL(bsg::k_pair_scan_apply, scan, dim3(bsg::kPairScanWidth), 0, p.d.stream, a);
        hipExtLaunchKernelGGL(bsg::k_pair_write, waves, dim3(bsg::kPairThreads), 0, p.d.stream, nullptr, kev.v[k + 1], 0, a);
        HIP_TRY(hipGetLastError());
        uint32_t *hdr = wp.rows->hdr + pair0;
        if (!direct) { staged_hdr.resize(n_pairs); hdr = staged_hdr.data(); }
        HIP_TRY(hipMemcpyAsync(hdr, d_phdr, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, p.d.stream));
        HIP_TRY(hipMemcpyAsync(&payload_len, d_poffs + n_pairs, 8, hipMemcpyDeviceToHost, p.d.stream));
        HIP_TRY(hipStreamSynchronize(p.d.stream));
        if (payload_len > 2 * part_words) return fail(BSG_E_HIP, "the list passes report %llu u32 of payload for %llu words",
                                                      (unsigned long long)payload_len, (unsigned long long)part_words);
        uint32_t *dst = wp.rows->payload;              // direct: every pair before the part's first has no rows, so no payload
        if (!direct) { staged_payload.resize(payload_len); dst = staged_payload.data(); }
        else if (payload_len > wp.rows->cap) return BSG_OK;                // the finish step reports it; no payload is written
        if (payload_len) HIP_TRY(hipMemcpyAsync(dst, d_payload, payload_len * 4, hipMemcpyDeviceToHost, p.d.stream));
        return BSG_OK;
    }
    // k_pair_hist between two events of the part's own (bsg_last_hist_ms, not bsg_last_match_ms), then the part's counters and
    // the scanner's list (the stream is waited for: its length sizes the copy)
    int32_t hist_results(PartDev &p)
    {
        HIP_TRY(hist_err);
        hist_dev = p.d.id;
        const WideHistOut &ho = *wp.hist;
        const uint32_t slots = ho.slots();
        if (n_pairs) {
            uint32_t max_tiles = 0;
            for (uint32_t ls = 0; ls < n_sets; ++ls)
                if (ps.pair_off[ls + 1] > ps.pair_off[ls]) max_tiles = std::max(max_tiles, bsh_wide::tiles_of(ps.first_row[ls + 1] - ps.first_row[ls]));
            // up to 64 waves per pair, each at least one step of tiles
            const uint32_t step = bsg::kPairHistStep;
            const uint32_t span_tiles = std::max(step, ((max_tiles + 63u) / 64u + step - 1u) / step * step);
            const uint32_t spans_max = std::max(1u, (max_tiles + span_tiles - 1u) / span_tiles);
            const uint64_t waves = (uint64_t)n_pairs * spans_max, per_block = bsg::kPairHistThreads / 64u;
            const uint64_t blocks = (waves + per_block - 1) / per_block;
            if (blocks > 0x7FFFFFFFull) return fail(BSG_E_UNSUPPORTED, "%llu (pair, span) waves on one device", (unsigned long long)waves);
            const size_t k = hev.v.size();
            HIP_TRY(hev.add(2));
            HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_pairs * slots * 4, p.d.stream));
            const bsg::PairHistArgs h{d_psets, d_sfirst, d_out, d_code, d_counts, n_pairs, n_sets, ho.n_buckets, span_tiles, spans_max};
            hipExtLaunchKernelGGL(bsg::k_pair_hist, dim3((uint32_t)blocks), dim3(bsg::kPairHistThreads), 0, p.d.stream, hev.v[k], hev.v[k + 1], 0, h);
            HIP_TRY(hipGetLastError());
            uint32_t *dst = ho.counts + (uint64_t)pair0 * slots;
            if (!direct) { staged_counts.resize((size_t)n_pairs * slots); dst = staged_counts.data(); }
            HIP_TRY(hipMemcpyAsync(dst, d_counts, (size_t)n_pairs * slots * 4, hipMemcpyDeviceToHost, p.d.stream));
        }
        uint32_t n = 0;
        HIP_TRY(hipMemcpyAsync(&n, d_nhfb, 4, hipMemcpyDeviceToHost, p.d.stream));
        HIP_TRY(hipStreamSynchronize(p.d.stream));
        if (n > p.n_rows) return fail(BSG_E_HIP, "the bucket scanner lists %u rows of %u", n, p.n_rows);
        hist_fb.resize(n);
        if (n) HIP_TRY(hipMemcpy(hist_fb.data(), d_hfb, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (uint32_t &r : hist_fb) r += p.r0;
        hist_ms = 0.f;
        for (size_t k = 0; k + 1 < hev.v.size(); k += 2) { float t = 0.f; (void)hipEventElapsedTime(&t, hev.v[k], hev.v[k + 1]); hist_ms += t; }
        return BSG_OK;
    }
    // the scanner's undecided rows join the walker's (GLOBAL indices): one list, each row once
    void more_fallback(std::vector<uint32_t> &fb)
    {
        if (hist_fb.empty()) return;
        fb.insert(fb.end(), hist_fb.begin(), hist_fb.end());
        std::sort(fb.begin(), fb.end());
        fb.erase(std::unique(fb.begin(), fb.end()), fb.end());
    }
    void landed()                                      // the part's layout -> the call's: per pair, the part's tiles of the set
    {
        if (direct || wp.rows || wp.hist) return;
        uint64_t at = 0;
        for (uint32_t ls = 0; ls < n_sets; ++ls) {
            const uint32_t s = ps.s0 + ls, tiles = bsh_wide::tiles_of(ps.first_row[ls + 1] - ps.first_row[ls]);
            const uint32_t set_tiles = bsh_wide::tiles_of(wp.set_first_row[s + 1] - wp.set_first_row[s]);
            for (uint32_t p = ps.pair_off[ls]; p < ps.pair_off[ls + 1] && tiles; ++p, at += tiles)
                memcpy(mc.out_bits + wp.set_word0[s] + (uint64_t)(p - wp.set_query_off[s]) * set_tiles + ps.tile0[ls], staged.data() + at, (size_t)tiles * 8);
        }
    }
};

// Rows [r0, r1) on one device, for every family: the rows' offsets rebased, the device's lock, scratch for rows / offsets / the
// condition table / programs / blob / fallback list, the conditions hashed and fingerprinted on the device, the rows uploaded in
// chunks (RowUpload) with one walker launch per chunk, the mode's results and the fallback rows back (GLOBAL indices), the
// kernels' time in *ms.  mode: PlanePart or WidePart.
template <class Mode>
int32_t match_part(bsg_ctx *ctx, Device &d, const MatchCall &mc, uint32_t r0, uint32_t r1, Mode &mode, std::vector<uint32_t> &fb, float *ms)
{
    const uint32_t n_rows = r1 - r0, n_conds = mc.n_conds;
    const uint64_t byte0 = mc.row_off[r0], n_bytes = mc.row_off[r1] - byte0;
    const LabTrace trace{mode.tag(), d.id};
    std::vector<uint64_t> local_off((size_t)n_rows + 1);                  // the run's offsets, relative to its first byte
    for (uint32_t r = 0; r <= n_rows; ++r) local_off[r] = mc.row_off[r0 + r] - byte0;
    if (int32_t rc = mode.plan(r0, r1)) return rc;
    d.calls.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(d.mu);
    if (int32_t rc = use_device(d)) return rc;
    if (int32_t rc = ensure_lower_table(d)) return rc;
    trace.lap(Mode::kPlanned);
    Scratch scratch(d);                                                   // every early return below leaves through it: drained, then freed
    PartDev p{d, scratch, r0, n_rows};
    uint8_t *d_rows = nullptr, *d_cbytes = nullptr;
    uint64_t *d_off = nullptr, *d_ch = nullptr, *d_cfp = nullptr;
    uint32_t *d_fb = nullptr, *d_nfb = nullptr, *d_coff = nullptr, *d_ckind = nullptr, *d_rx = nullptr;
    uint64_t *d_sub = nullptr;
    HIP_TRY(scratch.alloc(&d_rows, n_bytes + 64));
    HIP_TRY(scratch.alloc(&d_off, ((size_t)n_rows + 1) * 8));
    HIP_TRY(scratch.alloc(&d_ch, std::max<size_t>(n_conds, 1) * 2 * 32));
    HIP_TRY(scratch.alloc(&d_cfp, std::max<size_t>(n_conds, 1) * 2 * 8));
    HIP_TRY(scratch.alloc(&d_cbytes, (size_t)mc.cond_len + 64));
    HIP_TRY(scratch.alloc(&d_coff, ((size_t)2 * n_conds + 1) * 4));
    HIP_TRY(scratch.alloc(&d_ckind, std::max<size_t>(n_conds, 1) * 4));
    HIP_TRY(scratch.alloc(&p.d_prog, std::max<size_t>(mc.prog.size(), 1) * 4));
    if (mode.prog_off()) HIP_TRY(scratch.alloc(&p.d_poff, mc.prog_off.size() * 4));
    HIP_TRY(scratch.alloc(&d_fb, (size_t)n_rows * 4));
    HIP_TRY(scratch.alloc(&d_nfb, 4));
    if (mc.n_rx) HIP_TRY(scratch.alloc(&d_rx, mc.rx_blob.size() * 4));
    if (mc.substr) HIP_TRY(scratch.alloc(&d_sub, (size_t)bsg::kSubTableBytes));
    if (int32_t rc = mode.alloc(p)) return rc;
    trace.lap("device buffers allocated");
    HIP_TRY(hipMemsetAsync(d_rows + n_bytes, 0, 64, d.stream));
    HIP_TRY(hipMemcpyAsync(d_off, local_off.data(), ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, d.stream));
    if (n_conds) {
        // the condition strings are hashed AND fingerprinted (under the context's secret key) on the device
        if (mc.cond_len) HIP_TRY(hipMemcpyAsync(d_cbytes, mc.cond_bytes, mc.cond_len, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemsetAsync(d_cbytes + mc.cond_len, 0, 64, d.stream));
        HIP_TRY(hipMemcpyAsync(d_coff, mc.cond_off, ((size_t)2 * n_conds + 1) * 4, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemcpyAsync(d_ckind, mc.cond_kinds, (size_t)n_conds * 4, hipMemcpyHostToDevice, d.stream));
        hipLaunchKernelGGL(bsg::k_hash_fp_entries, dim3((2 * n_conds + 255) / 256), dim3(256), 0, d.stream, (const uint8_t *)d_cbytes,
                           (const uint32_t *)d_coff, 2 * n_conds, d_ch, d_cfp, ctx->fp_key);
        HIP_TRY(hipGetLastError());
        // a FieldRange condition has no token: lo and hi go where the hashes of its 17 bytes were written (the walkers' e[4], e[5])
        for (size_t i = 0; i < mc.range_conds.size(); ++i)
            HIP_TRY(hipMemcpyAsync(d_ch + ((size_t)2 * mc.range_conds[i] + 1) * 4, mc.range_bounds.data() + 2 * i, 16, hipMemcpyHostToDevice, d.stream));
    }
    if (!mc.prog.empty()) HIP_TRY(hipMemcpyAsync(p.d_prog, mc.prog.data(), mc.prog.size() * 4, hipMemcpyHostToDevice, d.stream));
    if (p.d_poff) HIP_TRY(hipMemcpyAsync(p.d_poff, mc.prog_off.data(), mc.prog_off.size() * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemsetAsync(d_nfb, 0, 4, d.stream));
    if (mc.n_rx) HIP_TRY(hipMemcpyAsync(d_rx, mc.rx_blob.data(), mc.rx_blob.size() * 4, hipMemcpyHostToDevice, d.stream));
    p.rx = bsg::RxArgs{d_rx, (uint32_t)mc.rx_blob.size(), mc.n_rx};
    if (mc.substr) {
        HIP_TRY(hipMemcpyAsync(d_sub, mc.sub.m.data(), (size_t)bsg::kSubTableBytes, hipMemcpyHostToDevice, d.stream));
        p.sub = bsg::SubArgs{d_sub, {mc.sub.start[0], mc.sub.start[1]}, {mc.sub.any[0], mc.sub.any[1]}};
    }
    p.d_ch = d_ch;
    // the three-consumer walkers copy the needle table and n_words of blob whatever the table holds: a table without a needle brings
    // its all-zero table, one without a regex condition no blob word at all
    if (mc.three() && (!mc.substr || !p.sub.table || (mc.n_rx == 0) != (p.rx.n_words == 0) || (p.rx.n_words != 0 && !p.rx.blob)))
        return fail(BSG_E_HIP, "%s: the needle table or the regex blob is not on the device", mode.tag());
    if (int32_t rc = mode.upload(p)) return rc;
    // The rows travel in chunks while the chunk before is being matched (RowUpload).  A surviving block is <= 10 MiB and goes in
    // one piece, in order on the one stream; a scan of many blocks in one call goes in pieces on the copy stream.
    RowUpload up(d, mc.rows + byte0, d_rows, local_off.data(), n_rows, ctx->ingest_chunk_bytes);
    const uint32_t n_chunks = up.n_chunks();
    HIP_TRY(up.start(n_chunks > 1));
    trace.lap("small uploads enqueued");
    HIP_TRY(up.copy(0));
    EventList kev;                                                       // per launch: kernel start, kernel stop
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t rf = up.cuts[c], re = up.cuts[c + 1];
        bsg::MatchArgs a{};
        a.rows = d_rows; a.row_off = d_off + rf; a.cond_h = d_ch; a.cond_fp = d_cfp; a.cond_kind = d_ckind; a.lower = d.d_lower;
        a.key = ctx->fp_key;
        a.fallback_rows = d_fb; a.n_fallback = d_nfb;
        a.n_rows = re - rf; a.row_base = rf; a.n_conds = n_conds;
        HIP_TRY(kev.add(2));
        HIP_TRY(up.wait_landed(c));
        mode.launch(p, a, rf, kev.v[(size_t)c * 2], kev.v[(size_t)c * 2 + 1]);
        HIP_TRY(hipGetLastError());
        if (c + 1 < n_chunks) HIP_TRY(up.copy(c + 1));                   // K(c) is running: now the next chunk's bytes
    }
    trace.lap("all chunks enqueued");
    uint32_t nfb = 0;
    if (int32_t rc = mode.results(p, kev)) return rc;
    HIP_TRY(hipMemcpyAsync(&nfb, d_nfb, 4, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    trace.lap(Mode::kBack);
    *ms = 0.f;
    for (size_t k = 0; k + 1 < kev.v.size(); k += 2) { float t = 0.f; (void)hipEventElapsedTime(&t, kev.v[k], kev.v[k + 1]); *ms += t; }
    fb.resize(nfb);
    if (nfb) HIP_TRY(hipMemcpy(fb.data(), d_fb, (size_t)nfb * 4, hipMemcpyDeviceToHost));
    for (uint32_t &r : fb) r += r0;
    mode.more_fallback(fb);
    scratch.done();                        // every kernel has finished, and each waited for its chunk's copy
    mode.landed();
    return BSG_OK;
}

// The validated, lowered call on the context's devices.
// Surviving blocks are independent (query_exec.go:729-764): a large scan is cut into one contiguous run of rows per
// device (bsh_wide::part_cuts over the call's sets: whole words of every result row, about equal bytes); a small one takes one
// device.  part(i, n_parts, device, r0, r1, fb, ms) runs one of them; their fallback rows are merged, sorted and handed out.
// finish() runs once every part has succeeded (bsg_match_rows_wide_rows: the stitch); the fallback list is handed out whatever it says.
template <class F, class G>
int32_t match_fan_out(bsg_ctx *ctx, const MatchCall &mc, const uint32_t *set_first_row, uint32_t n_sets, F &&part, G &&finish)
{
    const uint32_t nd = (uint32_t)ctx->devs.size();
    const uint32_t want = (nd > 1 && mc.n_bytes >= ctx->shard_min_row_bytes) ? nd : 1;
    const std::vector<uint32_t> cuts = bsh_wide::part_cuts(mc.row_off, mc.n_rows, set_first_row, n_sets, want);
    const uint32_t n_parts = (uint32_t)cuts.size() - 1;
    std::vector<std::vector<uint32_t>> fbs(n_parts);
    std::vector<float> ms(n_parts, 0.f);
    const uint32_t first = n_parts == 1 ? pick_device(ctx) : 0;
    if (int32_t rc = run_parts(n_parts, [&](uint32_t i) -> int32_t {
            return part(n_parts, *ctx->devs[(first + i) % nd], cuts[i], cuts[i + 1], fbs[i], &ms[i]);
        })) return rc;
    const int32_t finished = finish();
    std::vector<uint32_t> fb;
    for (auto &v : fbs) fb.insert(fb.end(), v.begin(), v.end());
    std::sort(fb.begin(), fb.end());
    *mc.out_n_fallback = (uint32_t)fb.size();
    if (!fb.empty() && mc.out_fallback_rows)
        memcpy(mc.out_fallback_rows, fb.data(), (size_t)std::min<uint32_t>((uint32_t)fb.size(), mc.fallback_cap) * 4);
    {
        std::lock_guard<std::shared_mutex> lk(ctx->mu);
        ctx->last_match_ms = *std::max_element(ms.begin(), ms.end());
    }
    if (fb.size() > mc.fallback_cap && mc.out_fallback_rows)
        return fail(BSG_E_INVALID, "%zu rows need the host matcher, caller's list holds %u", fb.size(), mc.fallback_cap);
    return finished;
}
template <class F>
int32_t match_fan_out(bsg_ctx *ctx, const MatchCall &mc, const uint32_t *set_first_row, uint32_t n_sets, F &&part)
{
    return match_fan_out(ctx, mc, set_first_row, n_sets, part, [] { return (int32_t)BSG_OK; });
}

// The call's route over its table (host/match_route.hpp), after begin_match_call: a refusal in the entry point's own words, else
// mc.route and the walker's slot.
int32_t route_call(MatchCall &mc, uint32_t n_queries)
{
    using bsh_route::Refusal;
    mc.route = bsh_route::route(*mc.call, mc.cond_kinds, mc.n_conds, n_queries);
    const uint32_t c = mc.route.cond, kind = mc.route.kind;
    switch (mc.route.refusal) {
    case Refusal::None: break;
    case Refusal::UnknownKind: return fail(BSG_E_INVALID, "condition %u: unknown kind %u", c, kind);
    case Refusal::RegexWithSubstr:
        return fail(BSG_E_UNSUPPORTED, "condition %u: a FieldRegex condition (regex and substring conditions share bsg_match_rows_regex_substr / bsg_match_rows_many_regex_substr)", c);
    case Refusal::TextWithRange:
        return fail(BSG_E_UNSUPPORTED, "condition %u: kind %u (the range calls hold Field, Token, FieldToken and FieldRange conditions)", c, kind);
    case Refusal::RegexInBatched:
        return fail(BSG_E_UNSUPPORTED, "condition %u: FieldRegex conditions are not matched by the batched call (use bsg_match_rows_regex)", c);
    }
    const bsh_route::Tok t = mc.default_tok ? bsh_route::Tok::Default : mc.spec.ngram != 0u ? bsh_route::Tok::Gram : bsh_route::Tok::Spec;
    mc.slot = bsh_route::slot(mc.call->mode, mc.route.consumers, t);
    return BSG_OK;
}

// The tables mc.route asks for, in the order blob, needle tables, range table (each rewrites cond_kinds from the current pointer).
// The batched calls' blob holds each regex condition's users (none for a batch without a query); the lookup call's is built over the
// DISTINCT regex conditions, under what this table's strings, pairs and lanes leave of a workgroup's 80 KiB.
int32_t build_tables(MatchCall &mc, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries, const bsh_lookup::Plan *lookup = nullptr)
{
    const bsh_route::Route &r = mc.route;
    if (r.blob) {
        std::vector<uint64_t> users;
        if (r.user_masks) users = n_queries ? bsh_rxg::user_masks(prog_ops, prog_off, n_queries, mc.n_conds) : std::vector<uint64_t>(mc.n_conds, 0);
        const uint32_t cap = r.cap == bsh_route::Cap::Lookup ? bsh_lookup::rx_lds_cap_of(lookup->n_strings(), (uint32_t)lookup->pairs.size()) : cap_bytes(r.cap);
        if (int32_t rc = build_rx_blob(mc.cond_bytes, mc.cond_off, mc.cond_kinds, mc.n_conds, mc.rx_blob, mc.n_rx, cap, r.user_masks ? users.data() : nullptr,
                                       lookup ? &lookup->rx_conds : nullptr)) return rc;
    }
    if (r.needles) if (int32_t rc = build_sub_tables(mc)) return rc;
    if (r.range_table) if (int32_t rc = build_range_table(mc)) return rc;
    return BSG_OK;
}

// the single and the batched calls' parts: planes over the implicit set {0, n_rows} (cuts at multiples of 64 rows)
int32_t match_planes_run(bsg_ctx *ctx, const MatchCall &mc, const ManyPlan *many)
{
    const uint32_t all_rows[2] = {0, mc.n_rows};
    return match_fan_out(ctx, mc, all_rows, 1, [&](uint32_t, Device &d, uint32_t r0, uint32_t r1, std::vector<uint32_t> &fb, float *ms) -> int32_t {
        PlanePart mode{mc, many};
        return match_part(ctx, d, mc, r0, r1, mode, fb, ms);
    });
}

// the single calls: the one-query case of the shared checks
int32_t match_rows_call(bsg_ctx *ctx, MatchCall &mc, const bsh_route::CallSpec &call, const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok_in)
{
    const uint32_t prog_off[2] = {0, n_ops};
    if (int32_t rc = begin_match_call(mc, call, kSingleFamily, tok_in, prog_ops, prog_off, 1)) return rc;
    if (int32_t rc = route_call(mc, 1)) return rc;
    if (int32_t rc = lower_programs(mc, kSingleFamily, prog_ops, prog_off, 1)) return rc;
    if (int32_t rc = build_tables(mc, prog_ops, prog_off, 1)) return rc;
    *mc.out_n_fallback = 0;
    if (mc.n_rows == 0) return BSG_OK;
    return match_planes_run(ctx, mc, nullptr);
}

// the batched calls: n_queries programs over one table of distinct conditions, one upload and one walk of the rows
int32_t match_rows_many_call(bsg_ctx *ctx, MatchCall &mc, const bsh_route::CallSpec &call, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                             const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok_in)
{
    if (int32_t rc = begin_match_call(mc, call, kManyFamily, tok_in, prog_ops, prog_off, n_queries)) return rc;
    if (int32_t rc = route_call(mc, n_queries)) return rc;
    const uint32_t n_rows = mc.n_rows;
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
    const ManyPlan plan{set_first_row, query_mask_of_set, n_sets, n_queries, ((size_t)n_rows + 63) / 64};
    if (int32_t rc = lower_programs(mc, kManyFamily, prog_ops, prog_off, n_queries)) return rc;
    if (int32_t rc = build_tables(mc, prog_ops, prog_off, n_queries)) return rc;
    if (n_queries == 0 || n_rows == 0) return BSG_OK;
    *mc.out_n_fallback = 0;
    return match_planes_run(ctx, mc, &plan);
}

// ---- bsg_match_rows_wide: any number of queries over one condition table (k_match_rows_store*, then k_eval_row_programs) ----
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

int32_t match_rows_wide_call(bsg_ctx *ctx, MatchCall &mc, const bsh_route::CallSpec &call, const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                             const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                             const bsg_tokenizer *tok_in, const WideRowsOut *rows = nullptr, const WideHistOut *hist = nullptr)
{
    const bool lookup = call.mode == bsh_route::Mode::Lookup, lookup_regex = lookup && call.accepts == bsh_route::Accepts::Regex;
    const Family &fam = lookup_regex ? kLookupRegexFamily : lookup ? kLookupFamily : kWideFamily;
    if (rows && (!rows->len || (rows->cap && !rows->payload))) return fail(BSG_E_INVALID, "null argument");
    if (int32_t rc = begin_match_call(mc, call, fam, tok_in, prog_ops, prog_off, n_queries)) return rc;
    const uint32_t n_rows = mc.n_rows;
    if (int32_t rc = route_call(mc, n_queries)) return rc;
    // the lookup call: the table's distinct role strings, their role records and the FieldToken pairs
    bsh_lookup::Plan lookup_plan;
    if (lookup) {
        uint32_t bad = 0;
        switch (bsh_lookup::build_strings(mc.cond_bytes, mc.cond_off, mc.cond_kinds, mc.n_conds, lookup_plan, &bad, lookup_regex)) {
        case bsh_lookup::Status::Ok: break;
        case bsh_lookup::Status::Kind:          // kinds above FieldRegex were refused as unknown
            return fail(BSG_E_UNSUPPORTED, "condition %u: FieldRegex conditions are not matched by the lookup call (use bsg_match_rows_wide)", bad);
        default: return fail(BSG_E_UNSUPPORTED, "%u conditions (the device matcher holds %u)", mc.n_conds, fam.max_conds);
        }
    }
    // the sets: the caller's, or one implicit set of all rows with every query
    WidePlan wp{set_first_row, set_query_off, set_queries, n_sets, n_queries, {}, {}, {}, rows, lookup ? &lookup_plan : nullptr, hist};
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
            return fail(BSG_E_UNSUPPORTED, "%u (set, query) pairs (one %s match call holds %u)", set_query_off[n_sets], fam.call, bsh_wide::kMaxPairs);
        if (set_query_off[n_sets] && !set_queries) return fail(BSG_E_INVALID, "set_queries is null");
        for (uint32_t s = 0; s < n_sets; ++s)
            for (uint32_t p = set_query_off[s]; p < set_query_off[s + 1]; ++p) {
                if (set_queries[p] >= n_queries) return fail(BSG_E_INVALID, "set %u lists query %u of %u", s, set_queries[p], n_queries);
                if (p > set_query_off[s] && set_queries[p] <= set_queries[p - 1])
                    return fail(BSG_E_INVALID, "set %u: its query list is not strictly ascending at pair %u", s, p);
            }
    }
    if (int32_t rc = lower_programs(mc, fam, prog_ops, prog_off, n_queries, lookup ? &lookup_plan.canon : nullptr)) return rc;
    if (int32_t rc = build_tables(mc, prog_ops, prog_off, n_queries, lookup ? &lookup_plan : nullptr)) return rc;
    const uint32_t n_pairs = wp.set_query_off[wp.n_sets];
    if (rows) {                                // every pair NONE until a part says otherwise (a set without rows lies in no part)
        if (n_pairs && !rows->hdr) return fail(BSG_E_INVALID, "null argument");
        if (n_pairs) memset(rows->hdr, 0, (size_t)n_pairs * 4);
        if (rows->off) memset(rows->off, 0, ((size_t)n_pairs + 1) * 8);
        *rows->len = 0;
    }
    if (n_rows == 0 || n_pairs == 0) return BSG_OK;
    // (the masks open regex conditions' DFAs: the lookup walker reads a u32 of regex slots per set instead, and none without regex conditions)
    if (lookup) wp.set_cond_mask.assign(wp.n_sets, 0);
    if (mc.n_rx && lookup) wp.set_rx_mask = bsh_lookup::set_rx_masks(lookup_plan, prog_ops, prog_off, n_queries, wp.set_query_off, wp.set_queries, wp.n_sets);
    else wp.set_cond_mask = bsh_wide::set_cond_masks(bsh_wide::query_cond_masks(prog_ops, prog_off, n_queries, mc.n_conds), wp.set_query_off, wp.set_queries, wp.n_sets);
    wp.set_word0.assign((size_t)wp.n_sets + 1, 0);
    for (uint32_t s = 0; s < wp.n_sets; ++s)
        wp.set_word0[s + 1] = wp.set_word0[s] + (uint64_t)bsh_wide::tiles_of(wp.set_first_row[s + 1] - wp.set_first_row[s]) *
                                                    (wp.set_query_off[s + 1] - wp.set_query_off[s]);
    *mc.out_n_fallback = 0;
    if (!rows && !hist)
        return match_fan_out(ctx, mc, wp.set_first_row, wp.n_sets,
                             [&](uint32_t n_parts, Device &d, uint32_t r0, uint32_t r1, std::vector<uint32_t> &fb, float *ms) -> int32_t {
                                 WidePart mode{mc, wp, n_parts == 1};
                                 return match_part(ctx, d, mc, r0, r1, mode, fb, ms);
                             });
    // the rows and the hist policies: the parts outlive their devices' work, the finish step makes the call's result of them (on one
    // thread, in any order)
    std::mutex kept_mu;
    std::vector<std::unique_ptr<WidePart>> kept;
    auto kept_part = [&](uint32_t n_parts, Device &d, uint32_t r0, uint32_t r1, std::vector<uint32_t> &fb, float *ms) -> int32_t {
        WidePart *mode = new WidePart{mc, wp, n_parts == 1};
        {
            std::lock_guard<std::mutex> lk(kept_mu);
            kept.emplace_back(mode);
        }
        return match_part(ctx, d, mc, r0, r1, *mode, fb, ms);
    };
    if (hist) {
        // every counter 0 until a part says otherwise (a set without rows lies in no part); the finish step adds the staged counters
        // of a set cut between parts
        const uint32_t slots = hist->slots();
        memset(hist->counts, 0, (size_t)n_pairs * slots * 4);
        return match_fan_out(ctx, mc, wp.set_first_row, wp.n_sets, kept_part, [&]() -> int32_t {
            float ms = 0.f;
            std::map<int, float> per_device;
            for (const auto &k : kept) {
                ms = std::max(ms, per_device[k->hist_dev] += k->hist_ms);
                if (k->direct) continue;
                uint32_t *dst = hist->counts + (uint64_t)k->pair0 * slots;
                for (size_t i = 0; i < k->staged_counts.size(); ++i) dst[i] += k->staged_counts[i];
            }
            std::lock_guard<std::shared_mutex> lk(ctx->mu);
            ctx->last_hist_ms = ms;
            return BSG_OK;
        });
    }
    return match_fan_out(ctx, mc, wp.set_first_row, wp.n_sets, kept_part, [&]() -> int32_t {
        uint64_t len = 0;
        std::vector<bsh_wide::PartRows> parts;
        if (kept.size() == 1) {                    // direct: the headers are the call's already, and the payload if it fits
            len = kept[0]->payload_len;
        } else {
            std::sort(kept.begin(), kept.end(), [](const auto &a, const auto &b) { return a->ps.s0 != b->ps.s0 ? a->ps.s0 < b->ps.s0 : a->ps.tile0[0] < b->ps.tile0[0]; });
            for (const auto &k : kept) {
                if (!k->n_pairs) continue;
                parts.push_back(bsh_wide::PartRows{&k->ps, k->staged_hdr.data(), k->staged_payload.data(), std::vector<uint64_t>((size_t)k->n_pairs + 1)});
                bsh_wide::pair_payload_offsets(parts.back().hdr, k->ps.first_row.data(), k->ps.pair_off.data(), k->n_sets, parts.back().off.data());
            }
            len = bsh_wide::stitch_headers(parts, wp.set_first_row, wp.set_query_off, wp.n_sets, rows->hdr);
        }
        *rows->len = len;
        if (rows->off) bsh_wide::pair_payload_offsets(rows->hdr, wp.set_first_row, wp.set_query_off, wp.n_sets, rows->off);
        if (len > rows->cap)
            return fail(BSG_E_INVALID, "the matches take %llu u32 of payload, caller's buffer holds %llu", (unsigned long long)len,
                        (unsigned long long)rows->cap);
        if (kept.size() != 1) bsh_wide::stitch_payloads(parts, wp.set_first_row, wp.set_query_off, wp.n_sets, rows->hdr, rows->payload);
        return BSG_OK;
    });
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
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kWide, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_wide_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                 const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                 const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                 const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                 const bsg_tokenizer *tok,
                                 uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                 uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    // (the shared checks ask for a result pointer with the rows: this call's is out_payload_len, the headers are asked for once the
    // pairs are counted; nothing is written through out_bits)
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_rows_wide_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                   const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                   const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                   const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                   const bsg_tokenizer *tok,
                                   uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideSubstr, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_wide_substr_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                        const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                        const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                        const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                        const bsg_tokenizer *tok,
                                        uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                        uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideSubstrRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_rows_wide_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                  const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                  const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                  const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                  const bsg_tokenizer *tok,
                                  uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideRange, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_wide_range_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                       const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                       const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                       const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                       const bsg_tokenizer *tok,
                                       uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                       uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideRangeRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_rows_wide_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                               const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                               const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                               const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                               const bsg_tokenizer *tok,
                                               uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideRegexSubstrRange, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_wide_regex_substr_range_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                                    const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                                    const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                                    const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                                    const bsg_tokenizer *tok,
                                                    uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                                    uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kWideRegexSubstrRangeRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_rows_wide_hist(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                 const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                 const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                 const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                 const bsg_tokenizer *tok,
                                 const uint8_t *field, uint32_t field_len, int64_t origin, uint64_t width, uint32_t n_buckets,
                                 uint32_t *out_counts, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    if (n_buckets == 0 || n_buckets > BSG_HIST_MAX_BUCKETS)
        return fail(BSG_E_INVALID, "n_buckets is %u (1 to %u)", n_buckets, BSG_HIST_MAX_BUCKETS);
    if (width == 0) return fail(BSG_E_INVALID, "width is 0");
    if (!field) return fail(BSG_E_INVALID, "field is null");
    if (field_len == 0 || field_len > BSG_MINMAX_MAX_NAME)
        return fail(BSG_E_INVALID, "field_len is %u (a name of 1 to %u bytes)", field_len, BSG_MINMAX_MAX_NAME);
    if (!out_counts) return fail(BSG_E_INVALID, "out_counts is null");
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, nullptr, out_fallback_rows, fallback_cap, out_n_fallback};   // the counters are the result (checked above)
    WideHistOut out{{}, origin, width, n_buckets, out_counts};
    memcpy(out.field.name, field, field_len);
    out.field.len = field_len;
    return match_rows_wide_call(ctx, mc, bsh_route::kWideHist, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, nullptr, &out);
}

int32_t bsg_last_hist_ms(bsg_ctx *ctx, float *hist_ms)
{
    BSG_ENTER(ctx);
    if (!hist_ms) return fail(BSG_E_INVALID, "null argument");
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    *hist_ms = ctx->last_hist_ms;
    return BSG_OK;
}

int32_t bsg_match_rows_lookup(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                              const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                              const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                              const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                              const bsg_tokenizer *tok,
                              uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kLookup, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_lookup_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                   const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                   const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                   const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                   const bsg_tokenizer *tok,
                                   uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                   uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kLookupRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_rows_lookup_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                    const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                    const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                    const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                    const bsg_tokenizer *tok,
                                    uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_wide_call(ctx, mc, bsh_route::kLookupRegex, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok);
}

int32_t bsg_match_rows_lookup_regex_rows(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                         const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                         const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                         const uint32_t *set_first_row, const uint32_t *set_query_off, const uint32_t *set_queries, uint32_t n_sets,
                                         const bsg_tokenizer *tok,
                                         uint32_t *out_pair_hdr, uint64_t *out_pair_off, uint32_t *out_payload, uint64_t payload_cap, uint64_t *out_payload_len,
                                         uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, reinterpret_cast<uint64_t *>(out_payload_len), out_fallback_rows,
                 fallback_cap, out_n_fallback};
    const WideRowsOut out{out_pair_hdr, out_pair_off, out_payload, payload_cap, out_payload_len};
    return match_rows_wide_call(ctx, mc, bsh_route::kLookupRegexRows, prog_ops, prog_off, n_queries, set_first_row, set_query_off, set_queries, n_sets, tok, &out);
}

int32_t bsg_match_pair_rows_list(uint32_t hdr, const uint32_t *payload, uint32_t set_rows, uint32_t *out_rows, uint32_t cap, uint32_t *out_n)
{
    switch (bsh_wide::pair_rows_list(hdr, payload, set_rows, out_rows, cap, out_n)) {
    case bsh_wide::ListStatus::Ok: return BSG_OK;
    case bsh_wide::ListStatus::Null: return fail(BSG_E_INVALID, "null argument");
    default: return fail(BSG_E_INVALID, "header 0x%08x and its payload are no pair of a set of %u rows", hdr, set_rows);
    }
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
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRows, prog_ops, n_ops, nullptr);
}

int32_t bsg_match_rows_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                             const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                             const uint32_t *prog_ops, uint32_t n_ops,
                             uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsRegex, prog_ops, n_ops, nullptr);
}

int32_t bsg_match_rows_tok(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                           const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                           const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                           uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsTok, prog_ops, n_ops, tok);
}

int32_t bsg_match_rows_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                              const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                              const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                              uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsSubstr, prog_ops, n_ops, tok);
}

int32_t bsg_match_rows_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                             const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                             const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                             uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsRange, prog_ops, n_ops, tok);
}

int32_t bsg_match_rows_many_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                  const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                  const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                  const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                  uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kManyRange, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
}

int32_t bsg_match_rows_many_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                   const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                   const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                   const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                   uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kManySubstr, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
}

int32_t bsg_match_rows_regex_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                    const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                    const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                    uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsRegexSubstr, prog_ops, n_ops, tok);
}

int32_t bsg_match_rows_many_regex_substr(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                         const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                         const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                         const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                         uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kManyRegexSubstr, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
}

int32_t bsg_match_rows_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                          const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                          const uint32_t *prog_ops, uint32_t n_ops, const bsg_tokenizer *tok,
                                          uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_call(ctx, mc, bsh_route::kRowsRegexSubstrRange, prog_ops, n_ops, tok);
}

int32_t bsg_match_rows_many_regex_substr_range(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                               const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                               const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                               const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                               uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kManyRegexSubstrRange, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
}

int32_t bsg_match_rows_many(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                            const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                            const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                            const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                            uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kMany, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
}

int32_t bsg_match_rows_many_regex(bsg_ctx *ctx, const uint8_t *rows, const uint64_t *row_off, uint32_t n_rows,
                                  const uint8_t *cond_bytes, const uint32_t *cond_off, const uint32_t *cond_kinds, uint32_t n_conds,
                                  const uint32_t *prog_ops, const uint32_t *prog_off, uint32_t n_queries,
                                  const uint32_t *set_first_row, const uint64_t *query_mask_of_set, uint32_t n_sets, const bsg_tokenizer *tok,
                                  uint64_t *out_bits, uint32_t *out_fallback_rows, uint32_t fallback_cap, uint32_t *out_n_fallback)
{
    BSG_ENTER(ctx);
    MatchCall mc{rows, row_off, n_rows, cond_bytes, cond_off, cond_kinds, n_conds, out_bits, out_fallback_rows, fallback_cap, out_n_fallback};
    return match_rows_many_call(ctx, mc, bsh_route::kManyRegex, prog_ops, prog_off, n_queries, set_first_row, query_mask_of_set, n_sets, tok);
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
