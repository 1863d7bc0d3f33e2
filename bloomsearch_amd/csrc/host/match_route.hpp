// match_route.hpp — which tables a row-matcher call builds and which walker serves it (match_api.inc), free of any device type.
// A CallSpec per public entry point says what the call accepts; route() reads the table's kinds and answers with a refusal or with
// the tables to build (regex blob and its LDS cap, needle tables, range table) and the walker's consumer set; slot() names one of
// the 60 walkers by (mode, consumer set, tokenizer), and BSH_MATCH_WALKERS lists the kernel of every slot: match_api.inc expands it
// into its launch table, tests/match_route_check.cpp into strings (tests/test_match_route.py).  DESIGN.md holds the route as a table.
#pragma once
#include <cstdint>

namespace bsh_route {

constexpr uint32_t kKindFieldToken = 2, kKindFieldRegex = 3, kKindSubstring = 4, kKindFieldSubstring = 5, kKindFieldRange = 6;   // bloomgpu.h BSG_KIND_*

enum class Mode : uint8_t { Single, Many, Wide, Lookup };           // planes of one query / of a batch; stored flags of the wide / lookup calls
enum class Consumers : uint8_t { None, Regex, Substr, RegexSubstr, Range, RegexSubstrRange };
enum class Tok : uint8_t { Default, Spec, Gram };                   // no tokenizer spec; a spec; a spec with an n-gram width
enum class Accepts : uint8_t {
    Plain,         // kinds 0-2
    Regex,         // kinds 0-3
    Substr,        // kinds 0-2, 4, 5; kind 3 is refused by name
    Range,         // kinds 0-2, 6; kinds 3-5 are refused by name
    RegexSubstr,   // kinds 0-5
    All,           // kinds 0-6: the table decides among RegexSubstr, Range and the three-consumer walkers
};
enum class Policy : uint8_t { Bits, Rows, Hist };                   // what a wide call hands back: words, tagged row lists, bucketed counts
enum class Cap : uint8_t { None, Single, SingleSub, Many, ManySub, Wide, WideSub, Lookup };
enum class Refusal : uint8_t { None, UnknownKind, RegexWithSubstr, TextWithRange, RegexInBatched };
enum class Status : uint8_t { Ok, Invalid, Unsupported };

constexpr bool has_regex(Consumers c) { return c == Consumers::Regex || c == Consumers::RegexSubstr || c == Consumers::RegexSubstrRange; }
constexpr bool has_substr(Consumers c) { return c == Consumers::Substr || c == Consumers::RegexSubstr || c == Consumers::RegexSubstrRange; }
constexpr bool has_range(Consumers c) { return c == Consumers::Range || c == Consumers::RegexSubstrRange; }

// the regex blob's LDS cap by name: regex_groups.hpp and wide_plan.hpp state the bytes (match_api.inc cap_bytes); Lookup is what the
// call's own lookup tables leave (lookup_plan.hpp rx_lds_cap_of)
constexpr Cap cap_of(Mode m, bool beside_needles)
{
    switch (m) {
    case Mode::Single: return beside_needles ? Cap::SingleSub : Cap::Single;
    case Mode::Many: return beside_needles ? Cap::ManySub : Cap::Many;
    case Mode::Wide: return beside_needles ? Cap::WideSub : Cap::Wide;
    default: return Cap::Lookup;
    }
}

struct CallSpec {
    const char *name;                  // the entry point
    Mode mode;
    Accepts accepts;
    Policy policy = Policy::Bits;
    const char *trace = name;          // the name in traces
    const char *trace_no_regex = trace;   // ... of a table without a FieldRegex condition
};
constexpr CallSpec with_policy(CallSpec s, Policy p, const char *name) { return CallSpec{name, s.mode, s.accepts, p, name, name}; }

constexpr CallSpec kRows{"bsg_match_rows", Mode::Single, Accepts::Plain};
constexpr CallSpec kRowsRegex{"bsg_match_rows_regex", Mode::Single, Accepts::Regex, Policy::Bits, "bsg_match_rows"};
constexpr CallSpec kRowsTok{"bsg_match_rows_tok", Mode::Single, Accepts::Regex, Policy::Bits, "bsg_match_rows"};
constexpr CallSpec kRowsSubstr{"bsg_match_rows_substr", Mode::Single, Accepts::Substr};
constexpr CallSpec kRowsRange{"bsg_match_rows_range", Mode::Single, Accepts::Range};
constexpr CallSpec kRowsRegexSubstr{"bsg_match_rows_regex_substr", Mode::Single, Accepts::RegexSubstr};
constexpr CallSpec kRowsRegexSubstrRange{"bsg_match_rows_regex_substr_range", Mode::Single, Accepts::All};
constexpr CallSpec kMany{"bsg_match_rows_many", Mode::Many, Accepts::Plain};
constexpr CallSpec kManyRegex{"bsg_match_rows_many_regex", Mode::Many, Accepts::Regex, Policy::Bits, "bsg_match_rows_many_regex", "bsg_match_rows_many"};
constexpr CallSpec kManySubstr{"bsg_match_rows_many_substr", Mode::Many, Accepts::Substr};
constexpr CallSpec kManyRange{"bsg_match_rows_many_range", Mode::Many, Accepts::Range};
constexpr CallSpec kManyRegexSubstr{"bsg_match_rows_many_regex_substr", Mode::Many, Accepts::RegexSubstr};
constexpr CallSpec kManyRegexSubstrRange{"bsg_match_rows_many_regex_substr_range", Mode::Many, Accepts::All};
constexpr CallSpec kWide{"bsg_match_rows_wide", Mode::Wide, Accepts::Regex};
constexpr CallSpec kWideRows = with_policy(kWide, Policy::Rows, "bsg_match_rows_wide_rows");
constexpr CallSpec kWideSubstr{"bsg_match_rows_wide_substr", Mode::Wide, Accepts::RegexSubstr};
constexpr CallSpec kWideSubstrRows = with_policy(kWideSubstr, Policy::Rows, "bsg_match_rows_wide_substr_rows");
constexpr CallSpec kWideRange{"bsg_match_rows_wide_range", Mode::Wide, Accepts::Range};
constexpr CallSpec kWideRangeRows = with_policy(kWideRange, Policy::Rows, "bsg_match_rows_wide_range_rows");
constexpr CallSpec kWideRegexSubstrRange{"bsg_match_rows_wide_regex_substr_range", Mode::Wide, Accepts::All};
constexpr CallSpec kWideRegexSubstrRangeRows = with_policy(kWideRegexSubstrRange, Policy::Rows, "bsg_match_rows_wide_regex_substr_range_rows");
constexpr CallSpec kWideHist = with_policy(kWideRegexSubstrRange, Policy::Hist, "bsg_match_rows_wide_hist");
constexpr CallSpec kLookup{"bsg_match_rows_lookup", Mode::Lookup, Accepts::Plain};
constexpr CallSpec kLookupRows = with_policy(kLookup, Policy::Rows, "bsg_match_rows_lookup_rows");
constexpr CallSpec kLookupRegex{"bsg_match_rows_lookup_regex", Mode::Lookup, Accepts::Regex};
constexpr CallSpec kLookupRegexRows = with_policy(kLookupRegex, Policy::Rows, "bsg_match_rows_lookup_regex_rows");

constexpr const CallSpec *kCallSpecs[] = {
    &kRows, &kRowsRegex, &kRowsTok, &kRowsSubstr, &kRowsRange, &kRowsRegexSubstr, &kRowsRegexSubstrRange,
    &kMany, &kManyRegex, &kManySubstr, &kManyRange, &kManyRegexSubstr, &kManyRegexSubstrRange,
    &kWide, &kWideRows, &kWideSubstr, &kWideSubstrRows, &kWideRange, &kWideRangeRows, &kWideRegexSubstrRange, &kWideRegexSubstrRangeRows, &kWideHist,
    &kLookup, &kLookupRows, &kLookupRegex, &kLookupRegexRows,
};

struct Route {
    Refusal refusal = Refusal::None;
    uint32_t cond = 0, kind = 0;       // a refusal: the first condition at fault and its kind
    bool blob = false;                 // build_rx_blob runs, under cap ...
    Cap cap = Cap::None;
    bool user_masks = false;           // ... with the batch's user masks
    bool needles = false;              // build_sub_tables runs
    bool range_table = false;          // build_range_table runs
    Consumers consumers = Consumers::None;
    const char *trace = nullptr;
    constexpr Status status() const
    {
        if (refusal == Refusal::None) return Status::Ok;
        return refusal == Refusal::UnknownKind ? Status::Invalid : Status::Unsupported;
    }
};

// The route of one call over a table of n_conds kinds.  Within one condition the checks run in the order regex-with-substr,
// text-with-range, regex-in-batched, unknown kind; the first condition at fault is the one named.  An Accepts::All call scans the whole
// table for unknown kinds first; a plain lookup call lets kind 3 pass: lookup_plan.hpp build_strings names its first FieldRegex condition.
inline Route route(const CallSpec &s, const uint32_t *kinds, uint32_t n_conds, uint32_t n_queries)
{
    Route r;
    auto refuse = [&r](Refusal why, uint32_t c, uint32_t kind) { r.refusal = why; r.cond = c; r.kind = kind; return r; };
    bool R = false, S = false, N = false;
    for (uint32_t c = 0; c < n_conds; ++c) {
        R |= kinds[c] == kKindFieldRegex;
        S |= kinds[c] == kKindSubstring || kinds[c] == kKindFieldSubstring;
        N |= kinds[c] == kKindFieldRange;
    }
    r.trace = R ? s.trace : s.trace_no_regex;
    const bool many = s.mode == Mode::Many, plain_lookup = s.mode == Mode::Lookup && s.accepts == Accepts::Plain;
    Accepts acc = s.accepts;
    if (acc == Accepts::All) {
        for (uint32_t c = 0; c < n_conds; ++c)
            if (kinds[c] > kKindFieldRange) return refuse(Refusal::UnknownKind, c, kinds[c]);
        if (!N) acc = Accepts::RegexSubstr;
        else if (!R && !S) acc = Accepts::Range;
    } else {
        const uint32_t max_kind = acc == Accepts::Plain ? (plain_lookup ? kKindFieldRegex : kKindFieldToken) : acc == Accepts::Regex ? kKindFieldRegex
                                  : acc == Accepts::Range ? kKindFieldRange : kKindFieldSubstring;
        for (uint32_t c = 0; c < n_conds; ++c) {
            const uint32_t k = kinds[c];
            if (acc == Accepts::Substr && k == kKindFieldRegex) return refuse(Refusal::RegexWithSubstr, c, k);
            if (acc == Accepts::Range && k >= kKindFieldRegex && k <= kKindFieldSubstring) return refuse(Refusal::TextWithRange, c, k);
            if (acc == Accepts::Plain && many && k == kKindFieldRegex) return refuse(Refusal::RegexInBatched, c, k);
            if (k > max_kind) return refuse(Refusal::UnknownKind, c, k);
        }
    }
    const bool blob_now = !many || n_queries != 0;     // a batch without a query launches nothing: its blob is not built
    switch (acc) {
    case Accepts::Plain: break;
    case Accepts::Regex:
        r.blob = blob_now; r.cap = cap_of(s.mode, false);
        r.consumers = R ? Consumers::Regex : Consumers::None;
        break;
    case Accepts::Substr:                              // the needle tables always, also for a table without a needle
        r.needles = true;
        r.consumers = Consumers::Substr;
        break;
    case Accepts::Range:
        r.range_table = true;
        r.consumers = N ? Consumers::Range : Consumers::None;
        break;
    case Accepts::RegexSubstr:                         // the blob beside a needle table only when the table holds a needle
        r.blob = blob_now; r.cap = cap_of(s.mode, S);
        r.needles = S;
        r.consumers = R && S ? Consumers::RegexSubstr : S ? Consumers::Substr : R ? Consumers::Regex : Consumers::None;
        break;
    case Accepts::All:                                 // kind 6 beside a text kind: the three tables in this order, needle or not, query or not
        r.blob = r.needles = r.range_table = true; r.cap = cap_of(s.mode, true);
        r.consumers = Consumers::RegexSubstrRange;
        break;
    }
    if (!r.blob) r.cap = Cap::None;
    r.user_masks = many && r.blob;
    return r;
}

// ---- the walkers: 3 modes x 6 consumer sets x 3 tokenizers, and the lookup mode's 2 x 3 ----
constexpr uint32_t kSetsPerMode = 6, kToks = 3, kLookupSlot0 = 3 * kSetsPerMode * kToks, kSlots = kLookupSlot0 + 2 * kToks, kNoSlot = ~0u;
constexpr uint32_t slot(Mode m, Consumers c, Tok t)
{
    if (m == Mode::Lookup) return (uint32_t)c > (uint32_t)Consumers::Regex ? kNoSlot : kLookupSlot0 + (uint32_t)c * kToks + (uint32_t)t;
    return ((uint32_t)m * kSetsPerMode + (uint32_t)c) * kToks + (uint32_t)t;
}
static_assert(kSlots == 60 && slot(Mode::Wide, Consumers::RegexSubstrRange, Tok::Gram) + 1 == kLookupSlot0 &&
              slot(Mode::Lookup, Consumers::Regex, Tok::Gram) + 1 == kSlots && slot(Mode::Lookup, Consumers::Substr, Tok::Default) == kNoSlot);

}  // namespace bsh_route

// One line per walker: X(mode, consumer set, tokenizer, kernel of match.hip.h / match_lookup.hip.h).
#define BSH_MATCH_WALKERS(X) \
    X(Single, None, Default, k_match_rows)                                      \
    X(Single, None, Spec, k_match_rows_tok)                                     \
    X(Single, None, Gram, k_match_rows_gram)                                    \
    X(Single, Regex, Default, k_match_rows_regex)                               \
    X(Single, Regex, Spec, k_match_rows_regex_tok)                              \
    X(Single, Regex, Gram, k_match_rows_regex_gram)                             \
    X(Single, Substr, Default, k_match_rows_substr)                             \
    X(Single, Substr, Spec, k_match_rows_substr_tok)                            \
    X(Single, Substr, Gram, k_match_rows_substr_gram)                           \
    X(Single, RegexSubstr, Default, k_match_rows_regex_substr)                  \
    X(Single, RegexSubstr, Spec, k_match_rows_regex_substr_tok)                 \
    X(Single, RegexSubstr, Gram, k_match_rows_regex_substr_gram)                \
    X(Single, Range, Default, k_match_rows_range)                               \
    X(Single, Range, Spec, k_match_rows_range_tok)                              \
    X(Single, Range, Gram, k_match_rows_range_gram)                             \
    X(Single, RegexSubstrRange, Default, k_match_rows_regex_substr_range)       \
    X(Single, RegexSubstrRange, Spec, k_match_rows_regex_substr_range_tok)      \
    X(Single, RegexSubstrRange, Gram, k_match_rows_regex_substr_range_gram)     \
    X(Many, None, Default, k_match_rows_many)                                   \
    X(Many, None, Spec, k_match_rows_many_tok)                                  \
    X(Many, None, Gram, k_match_rows_many_gram)                                 \
    X(Many, Regex, Default, k_match_rows_many_regex)                            \
    X(Many, Regex, Spec, k_match_rows_many_regex_tok)                           \
    X(Many, Regex, Gram, k_match_rows_many_regex_gram)                          \
    X(Many, Substr, Default, k_match_rows_many_substr)                          \
    X(Many, Substr, Spec, k_match_rows_many_substr_tok)                         \
    X(Many, Substr, Gram, k_match_rows_many_substr_gram)                        \
    X(Many, RegexSubstr, Default, k_match_rows_many_regex_substr)               \
    X(Many, RegexSubstr, Spec, k_match_rows_many_regex_substr_tok)              \
    X(Many, RegexSubstr, Gram, k_match_rows_many_regex_substr_gram)             \
    X(Many, Range, Default, k_match_rows_many_range)                            \
    X(Many, Range, Spec, k_match_rows_many_range_tok)                           \
    X(Many, Range, Gram, k_match_rows_many_range_gram)                          \
    X(Many, RegexSubstrRange, Default, k_match_rows_many_regex_substr_range)    \
    X(Many, RegexSubstrRange, Spec, k_match_rows_many_regex_substr_range_tok)   \
    X(Many, RegexSubstrRange, Gram, k_match_rows_many_regex_substr_range_gram)  \
    X(Wide, None, Default, k_match_rows_store)                                  \
    X(Wide, None, Spec, k_match_rows_store_tok)                                 \
    X(Wide, None, Gram, k_match_rows_store_gram)                                \
    X(Wide, Regex, Default, k_match_rows_store_regex)                           \
    X(Wide, Regex, Spec, k_match_rows_store_regex_tok)                          \
    X(Wide, Regex, Gram, k_match_rows_store_regex_gram)                         \
    X(Wide, Substr, Default, k_match_rows_store_substr)                         \
    X(Wide, Substr, Spec, k_match_rows_store_substr_tok)                        \
    X(Wide, Substr, Gram, k_match_rows_store_substr_gram)                       \
    X(Wide, RegexSubstr, Default, k_match_rows_store_regex_substr)              \
    X(Wide, RegexSubstr, Spec, k_match_rows_store_regex_substr_tok)             \
    X(Wide, RegexSubstr, Gram, k_match_rows_store_regex_substr_gram)            \
    X(Wide, Range, Default, k_match_rows_store_range)                           \
    X(Wide, Range, Spec, k_match_rows_store_range_tok)                          \
    X(Wide, Range, Gram, k_match_rows_store_range_gram)                         \
    X(Wide, RegexSubstrRange, Default, k_match_rows_store_regex_substr_range)   \
    X(Wide, RegexSubstrRange, Spec, k_match_rows_store_regex_substr_range_tok)  \
    X(Wide, RegexSubstrRange, Gram, k_match_rows_store_regex_substr_range_gram) \
    X(Lookup, None, Default, k_match_rows_lookup)                               \
    X(Lookup, None, Spec, k_match_rows_lookup_tok)                              \
    X(Lookup, None, Gram, k_match_rows_lookup_gram)                             \
    X(Lookup, Regex, Default, k_match_rows_lookup_regex)                        \
    X(Lookup, Regex, Spec, k_match_rows_lookup_regex_tok)                       \
    X(Lookup, Regex, Gram, k_match_rows_lookup_regex_gram)
