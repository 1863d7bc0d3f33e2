// substring_groups.hpp — the arithmetic of substring conditions in a group of batched queries, free of any device type: would
// the next query's needles still pack beside the group's (the first-fit of substring_pack.hpp pack_needles, needle by needle in
// condition order), do the group's regex tables still fit beside a needle table (the reduced caps of regex_groups.hpp, from the
// first needle on), and which device call decides a group.  The engine mirror (engine.hpp match_rows_device_many) closes its groups
// and picks its entry points by these functions; tests/substring_groups_check.cpp runs the same code on the CPU
// (tests/test_substring_groups.py).
#pragma once
#include <cstdint>
#include <vector>

#include "regex_groups.hpp"
#include "substring_pack.hpp"
#include "wide_plan.hpp"

namespace bsh_subg {

// The words of one call's needle table as pack_needles fills them: a needle goes into the first word with room for all of it.
// place() is one step of that loop, so placing a group's needles one by one, in condition order, answers exactly as pack_needles
// over all of them does.
struct NeedleBins {
    uint32_t used[bsh::kSubWords] = {};
    bool place(uint32_t n)
    {
        if (n == 0 || n > bsh::kSubMaxNeedle) return false;
        uint32_t w = 0;
        while (w < bsh::kSubWords && used[w] + n > 64u) ++w;
        if (w == bsh::kSubWords) return false;
        used[w] += n;
        return true;
    }
};

// the bytes a group's regex tables may take: the call's own cap, the reduced one once the table holds a needle
inline uint32_t regex_table_cap(bool wide, bool needles)
{
    if (wide) return needles ? bsh_rxg::kWideSubLdsCap : bsh_wide::kWideLdsCap;
    return needles ? bsh_rxg::kManySubLdsCap : bsh_rxg::kManyLdsCap;
}

// What a group holds of the two text consumers, and what the next query would add: the folded lengths of its fresh substring
// conditions in condition order, and the estimated table bytes (regex_groups.hpp rx_table_bytes) of its fresh regex conditions.
struct Group {
    NeedleBins bins;
    uint32_t n_needles = 0, rx_bytes = 0;
};
struct Fresh {
    std::vector<uint32_t> needle_len;
    uint32_t rx_bytes = 0;
};

// Would the group still be one call with the query in it: every fresh needle finds its word, and the regex tables of both stay
// within the cap — the reduced cap exactly when the group or the query holds a needle.
inline bool fits(const Group &g, const Fresh &f, bool wide)
{
    NeedleBins bins = g.bins;
    for (const uint32_t n : f.needle_len)
        if (!bins.place(n)) return false;
    const bool needles = g.n_needles + f.needle_len.size() != 0;
    return bsh_rxg::align4(g.rx_bytes + f.rx_bytes) <= regex_table_cap(wide, needles);
}
inline void add(Group &g, const Fresh &f)
{
    for (const uint32_t n : f.needle_len) (void)g.bins.place(n);
    g.n_needles += (uint32_t)f.needle_len.size();
    g.rx_bytes += f.rx_bytes;
}

// The call that decides a group, by what its table holds and the engine's wide keys (wide_rows implies wide).  A group with a needle
// never takes a lookup call: under the lookup keys it is the wide route's.
enum class Call : uint8_t { Many, ManyRegex, ManySubstr, ManyRegexSubstr, Wide, WideRows, WideSubstr, WideSubstrRows };
inline Call group_call(bool regex, bool needles, bool wide, bool wide_rows)
{
    if (wide || wide_rows) return needles ? (wide_rows ? Call::WideSubstrRows : Call::WideSubstr) : (wide_rows ? Call::WideRows : Call::Wide);
    if (needles) return regex ? Call::ManyRegexSubstr : Call::ManySubstr;
    return regex ? Call::ManyRegex : Call::Many;
}
inline const char *call_name(Call c)
{
    switch (c) {
    case Call::Many: return "bsg_match_rows_many";
    case Call::ManyRegex: return "bsg_match_rows_many_regex";
    case Call::ManySubstr: return "bsg_match_rows_many_substr";
    case Call::ManyRegexSubstr: return "bsg_match_rows_many_regex_substr";
    case Call::Wide: return "bsg_match_rows_wide";
    case Call::WideRows: return "bsg_match_rows_wide_rows";
    case Call::WideSubstr: return "bsg_match_rows_wide_substr";
    default: return "bsg_match_rows_wide_substr_rows";
    }
}

}  // namespace bsh_subg
