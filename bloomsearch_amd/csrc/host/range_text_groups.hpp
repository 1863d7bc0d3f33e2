// range_text_groups.hpp — the arithmetic of groups that hold range conditions BESIDE regex and substring ones
// (bsg_match_rows_many_regex_substr_range), free of any device type.  Under the engine's DeviceMatchRangeText key, and with no wide or
// lookup key set, bse_query_many lets the two families share a group: may the next query join, which bytes may the group's regex tables
// take (the reduced cap beside a needle table as soon as kind 6 sits beside ANY text condition, needle or not: the three-consumer
// walkers always carry the needle table), does the group with the query in it stay within every limit of the one call, and which call
// decides it.  Without the key, and under a wide or lookup key, every answer is range_groups.hpp's and substring_groups.hpp's,
// unchanged (range_groups.hpp itself is untouched: tests/test_range_groups.py pins joins).  The engine mirror (engine.hpp
// match_rows_device_many) closes its groups and picks its entry points by these functions; tests/range_text_groups_check.cpp runs the
// same code on the CPU (tests/test_range_text_groups.py).
// Under a wide or lookup key the two families share a group only with the DeviceMatchRangeTextWide key as well: the wide_* functions at
// the end (bsg_match_rows_wide_regex_substr_range(_rows); tests/range_text_wide_groups_check.cpp, tests/test_range_text_wide_groups.py).
#pragma once
#include <cstdint>
#include <string_view>
#include <vector>

#include "range_groups.hpp"

namespace bsh_rtg {

using bsh_rngg::Mix;

constexpr uint32_t kMaxQueries = 64, kMaxConds = 64;            // bloomgpu.h bsg_match_rows_many: one mask bit per query, one flag per condition
constexpr uint32_t kMixedCap = bsh_rxg::kManySubLdsCap;         // 34 032: regex tables (user masks included) of a mixed group

// May range and text conditions share a group at all: the key, DeviceMatch, and none of the wide / lookup keys (wide = any of them).
inline bool mixing(bool device_match, bool range_text_key, bool wide) { return device_match && range_text_key && !wide; }

// Would the group still be one call with the query in it, as far as the two families go: always where they may mix, else
// range_groups.hpp's rule (kind 6 never meets kinds 3-5, whichever came first).
inline bool joins(bool mix_ok, const Mix &group, const Mix &query) { return mix_ok || bsh_rngg::joins(group, query); }

// A table with kind 6 beside a kind 3-5 condition: the three-consumer walkers decide it.
inline bool mixed(const Mix &m) { return m.range && m.text; }
inline Mix with(const Mix &group, const Mix &query)
{
    Mix m = group;
    bsh_rngg::add(m, query);
    return m;
}

// The bytes a group's regex tables may take: the reduced cap for a mixed table whether or not it holds a needle, else what
// substring_groups.hpp says (base: the call's own cap, e.g. the lookup regex call's; it never applies to a mixed group).
inline uint32_t regex_table_cap(const Mix &table, bool wide, bool needles, uint32_t base)
{
    if (mixed(table)) return kMixedCap;
    return needles ? bsh_subg::regex_table_cap(wide, true) : base;
}

// What a non-wide group holds, and what the next query would add to it.
struct Group {
    Mix mix;
    bsh_subg::Group sub;                                        // its needles as they pack, and the bytes of its regex tables
    uint32_t n_queries = 0, n_conds = 0, n_rx = 0;
};
struct Fresh {
    Mix mix;
    bsh_subg::Fresh sub;                                        // the folded lengths of its fresh needles, the bytes of its fresh regex tables
    uint32_t n_conds = 0, n_rx = 0;                             // its fresh distinct conditions, the regex ones among them
    uint32_t query_conds = 0;                                   // all conditions of the query alone
    uint32_t co_active = 0;                                     // regex_groups.hpp co_active_bound over the group's and the query's regex fields
};

// Every closing rule of a batched (non-wide) group at once: 64 queries, 64 conditions, 16 regex conditions, co_active_bound, needles
// that pack first-fit, and the regex-table estimate against the cap the table with the query in it has.
inline bool fits(bool mix_ok, const Group &g, const Fresh &f)
{
    if (!joins(mix_ok, g.mix, f.mix)) return false;
    if (g.n_queries + 1 > kMaxQueries || f.query_conds > kMaxConds || g.n_conds + f.n_conds > kMaxConds) return false;
    if (g.n_rx + f.n_rx > bsh_rxg::kMaxRegexConds || f.co_active > bsh_rxg::kManySlots) return false;
    const bool needles = g.sub.n_needles + f.sub.needle_len.size() != 0;
    if (needles && !bsh_subg::fits(g.sub, f.sub, false)) return false;
    return bsh_rxg::align4(g.sub.rx_bytes + f.sub.rx_bytes) <= regex_table_cap(with(g.mix, f.mix), false, needles, bsh_rxg::kManyLdsCap);
}
inline void add(Group &g, const Fresh &f)
{
    bsh_rngg::add(g.mix, f.mix);
    bsh_subg::add(g.sub, f.sub);
    ++g.n_queries;
    g.n_conds += f.n_conds;
    g.n_rx += f.n_rx;
}

constexpr const char *kManyCall = "bsg_match_rows_many_regex_substr_range";
// The entry point of a group that no lookup call decides: the one new call for a mixed table (there is none under a wide key: such a
// group never forms), else range_groups.hpp's answer.
inline const char *group_call_name(const Mix &table, bool regex, bool needles, bool wide, bool wide_rows)
{
    if (mixed(table)) return wide || wide_rows ? nullptr : kManyCall;
    return bsh_rngg::group_call_name(table.range, regex, needles, wide, wide_rows);
}

// ---- under a wide or lookup key: the engine's DeviceMatchRangeTextWide key (bsg_match_rows_wide_regex_substr_range(_rows)) ----
// Every answer above stands as it is; these are asked beside them.

// May range and text conditions share a group under a wide or lookup key (wide = any of them): DeviceMatch, DeviceMatchRangeText and the
// wide key of the two families.
inline bool wide_mixing(bool device_match, bool range_text_key, bool range_text_wide_key, bool wide)
{
    return device_match && range_text_key && range_text_wide_key && wide;
}

constexpr uint32_t kWideMixedCap = bsh_rxg::kWideSubLdsCap;     // 42 496: regex tables (no user masks) of a mixed wide group, needle or not
// The bytes the regex tables of a wide group may take: the cap beside the needle table for a mixed table whether or not it holds a
// needle (the three-consumer storing walkers always carry the needle table), else what regex_table_cap says of a wide group.
inline uint32_t wide_regex_table_cap(const Mix &table, bool needles, uint32_t base)
{
    if (mixed(table)) return kWideMixedCap;
    return regex_table_cap(table, true, needles, base);
}

// Every closing rule of a wide group at once.  No member limit beyond the call's own (bsh_wide::kMaxQueries); 64 conditions, 16 regex
// conditions, co_active_bound, needles that pack by substring_groups.hpp fits(.., wide = true), and the regex-table estimate against
// the cap the table with the query in it has (base: the cap of a table without a needle and not mixed, the wide call's own).
inline bool wide_fits(bool mix_ok, const Group &g, const Fresh &f, uint32_t base = bsh_wide::kWideLdsCap)
{
    if (!joins(mix_ok, g.mix, f.mix)) return false;
    if (g.n_queries + 1 > bsh_wide::kMaxQueries || f.query_conds > kMaxConds || g.n_conds + f.n_conds > kMaxConds) return false;
    if (g.n_rx + f.n_rx > bsh_rxg::kMaxRegexConds || f.co_active > bsh_rxg::kManySlots) return false;
    const bool needles = g.sub.n_needles + f.sub.needle_len.size() != 0;
    if (needles && !bsh_subg::fits(g.sub, f.sub, true)) return false;
    return bsh_rxg::align4(g.sub.rx_bytes + f.sub.rx_bytes) <= wide_regex_table_cap(with(g.mix, f.mix), needles, base);
}

constexpr const char *kWideCall = "bsg_match_rows_wide_regex_substr_range", *kWideRowsCall = "bsg_match_rows_wide_regex_substr_range_rows";
// The entry point of a wide group that no lookup call decides: the new call (its _rows twin under a rows key) for a mixed table, else
// group_call_name's answer.
inline const char *wide_group_call_name(const Mix &table, bool regex, bool needles, bool wide_rows)
{
    if (mixed(table)) return wide_rows ? kWideRowsCall : kWideCall;
    return group_call_name(table, regex, needles, true, wide_rows);
}

}  // namespace bsh_rtg
