// range_groups.hpp — the arithmetic of range conditions in a group of batched queries, free of any device type: may the next query
// join a group (a table never holds a FieldRange condition beside a FieldRegex, Substring or FieldSubstring one: no walker takes
// both), may a group hold the lookup calls' 1 024 conditions, and which device call decides a group.  For a group without a range
// condition every answer is substring_groups.hpp's, unchanged.  The engine mirror (engine.hpp match_rows_device_many) closes its groups
// and picks its entry points by these functions; tests/range_groups_check.cpp runs the same code on the CPU
// (tests/test_range_groups.py).
#pragma once
#include <cstdint>

#include "substring_groups.hpp"

namespace bsh_rngg {

constexpr uint32_t kKindFieldRegex = 3, kKindSubstring = 4, kKindFieldSubstring = 5, kKindFieldRange = 6;   // bloomgpu.h BSG_KIND_*

// What a table (a group's, or the one a query alone would make) holds of the two families that exclude each other: a range
// condition, and a condition of a text consumer.  Field / Token / FieldToken conditions belong to neither and go with both.
struct Mix {
    bool range = false, text = false;
    void see(uint32_t kind)
    {
        range = range || kind == kKindFieldRange;
        text = text || (kind >= kKindFieldRegex && kind <= kKindFieldSubstring);
    }
};
inline bool valid(const Mix &m) { return !(m.range && m.text); }
// Would the group still be one call with the query in it: kind 6 never meets kinds 3-5, whichever of the two came first.
inline bool joins(const Mix &group, const Mix &query) { return !((group.range || query.range) && (group.text || query.text)); }
inline void add(Mix &group, const Mix &query)
{
    group.range = group.range || query.range;
    group.text = group.text || query.text;
}

// Under the lookup keys: may the group grow to the lookup calls' 1 024 conditions (and be decided by one of them)?  Never with a
// range condition or a needle; with a regex condition only under the lookup regex key.
inline bool lookup_group(bool lookup, bool lookup_regex, bool range, bool regex, bool needles)
{
    return lookup && !range && !needles && (!regex || lookup_regex);
}

// The call that decides a group WITH a range condition, by the engine's wide keys (wide_rows implies wide; the lookup keys imply wide
// too: such a group takes the wide route, bounded by 64 conditions, as a group with a needle does).
enum class Call : uint8_t { ManyRange, WideRange, WideRangeRows };
inline Call range_group_call(bool wide, bool wide_rows)
{
    if (wide || wide_rows) return wide_rows ? Call::WideRangeRows : Call::WideRange;
    return Call::ManyRange;
}
inline const char *call_name(Call c)
{
    switch (c) {
    case Call::ManyRange: return "bsg_match_rows_many_range";
    case Call::WideRange: return "bsg_match_rows_wide_range";
    default: return "bsg_match_rows_wide_range_rows";
    }
}

// The entry point of a group that no lookup call decides, whatever it holds: the range calls with a range condition, else exactly
// what substring_groups.hpp names.  nullptr: no call decides a table with both families (joins() keeps such a group from forming).
inline const char *group_call_name(bool range, bool regex, bool needles, bool wide, bool wide_rows)
{
    if (range) return regex || needles ? nullptr : call_name(range_group_call(wide, wide_rows));
    return bsh_subg::call_name(bsh_subg::group_call(regex, needles, wide, wide_rows));
}

}  // namespace bsh_rngg
