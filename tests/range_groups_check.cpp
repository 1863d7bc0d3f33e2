// range_groups_check.cpp — runs bloomsearch_amd/csrc/host/range_groups.hpp on the CPU for tests/test_range_groups.py.
//   range_groups_check <cases.txt> <answers.txt>
// One case per line, one answer line per case:
//   G (<kind>[,<kind>]* | -)...                     -> per query (the kinds of its conditions, - for none), added in order to ONE group:
//                                                      1 = joins() took it (then add()), 0 = refused (the group stays as it was)
//   K <range> <regex> <needles> <wide> <wide_rows>  -> the name of the call group_call_name chooses, - for none
//   S <regex> <needles> <wide> <wide_rows>          -> the name substring_groups.hpp's group_call chooses (the answer of a group without ranges)
//   L <lookup> <lookup_regex> <range> <regex> <needles>   -> 1 = the group may hold the lookup calls' conditions and take one of them
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "host/range_groups.hpp"

static bsh_rngg::Mix mix_of(const std::string &kinds)
{
    bsh_rngg::Mix m;
    if (kinds == "-") return m;
    std::istringstream ks(kinds);
    std::string k;
    while (std::getline(ks, k, ',')) m.see((uint32_t)std::stoul(k));
    return m;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.txt answers.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        ls >> kind;
        if (kind == "G") {
            bsh_rngg::Mix group;
            std::string kinds;
            bool first = true;
            while (ls >> kinds) {
                const bsh_rngg::Mix q = mix_of(kinds);
                const bool ok = bsh_rngg::valid(q) && bsh_rngg::joins(group, q);
                if (ok) bsh_rngg::add(group, q);
                out << (first ? "" : " ") << (ok ? 1 : 0);
                first = false;
            }
            out << "\n";
        } else if (kind == "K") {
            uint32_t range = 0, regex = 0, needles = 0, wide = 0, wide_rows = 0;
            ls >> range >> regex >> needles >> wide >> wide_rows;
            const char *name = bsh_rngg::group_call_name(range != 0, regex != 0, needles != 0, wide != 0, wide_rows != 0);
            out << (name ? name : "-") << "\n";
        } else if (kind == "S") {
            uint32_t regex = 0, needles = 0, wide = 0, wide_rows = 0;
            ls >> regex >> needles >> wide >> wide_rows;
            out << bsh_subg::call_name(bsh_subg::group_call(regex != 0, needles != 0, wide != 0, wide_rows != 0)) << "\n";
        } else if (kind == "L") {
            uint32_t lookup = 0, lookup_regex = 0, range = 0, regex = 0, needles = 0;
            ls >> lookup >> lookup_regex >> range >> regex >> needles;
            out << (bsh_rngg::lookup_group(lookup != 0, lookup_regex != 0, range != 0, regex != 0, needles != 0) ? 1 : 0) << "\n";
        } else {
            std::fprintf(stderr, "unknown case %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
