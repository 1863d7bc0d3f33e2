// range_text_wide_groups_check.cpp — runs the wide part of bloomsearch_amd/csrc/host/range_text_groups.hpp on the CPU for
// tests/test_range_text_wide_groups.py.
//   range_text_wide_groups_check <cases.txt> <answers.txt>
// One case per line, one answer line per case:
//   M <device_match> <key> <wide key> <wide>    -> 1 = range and text conditions may share a group under a wide or lookup key
//   C <range> <text> <needles> <base>           -> the bytes the regex tables of such a wide table may take
//   K <range> <text> <regex> <needles> <wide_rows> -> the name of the call wide_group_call_name chooses, - for none
//   F <mix_ok> <query>...                       -> per query, added in order to ONE wide group: 1 = wide_fits() took it (then add()),
//                                                  0 = refused (the group stays as it was)
//     <query> = kinds/needle lengths/regex table bytes/fresh conditions/fresh regex conditions/conditions of the query/co_active,
//               the first two comma lists or -
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/range_text_groups.hpp"

static std::vector<uint32_t> list_of(const std::string &s)
{
    std::vector<uint32_t> v;
    if (s == "-") return v;
    std::istringstream is(s);
    std::string k;
    while (std::getline(is, k, ',')) v.push_back((uint32_t)std::stoul(k));
    return v;
}

static bsh_rtg::Fresh fresh_of(const std::string &q)
{
    std::vector<std::string> part;
    std::istringstream is(q);
    std::string p;
    while (std::getline(is, p, '/')) part.push_back(p);
    bsh_rtg::Fresh f;
    if (part.size() != 7) { std::fprintf(stderr, "bad query %s\n", q.c_str()); std::exit(2); }
    for (const uint32_t k : list_of(part[0])) f.mix.see(k);
    f.sub.needle_len = list_of(part[1]);
    f.sub.rx_bytes = (uint32_t)std::stoul(part[2]);
    f.n_conds = (uint32_t)std::stoul(part[3]);
    f.n_rx = (uint32_t)std::stoul(part[4]);
    f.query_conds = (uint32_t)std::stoul(part[5]);
    f.co_active = (uint32_t)std::stoul(part[6]);
    return f;
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
        if (kind == "M") {
            int dm = 0, key = 0, wide_key = 0, wide = 0;
            ls >> dm >> key >> wide_key >> wide;
            out << (bsh_rtg::wide_mixing(dm != 0, key != 0, wide_key != 0, wide != 0) ? 1 : 0) << "\n";
        } else if (kind == "C") {
            int range = 0, text = 0, needles = 0;
            uint32_t base = 0;
            ls >> range >> text >> needles >> base;
            bsh_rtg::Mix m;
            m.range = range != 0; m.text = text != 0;
            out << bsh_rtg::wide_regex_table_cap(m, needles != 0, base) << "\n";
        } else if (kind == "K") {
            int range = 0, text = 0, regex = 0, needles = 0, wide_rows = 0;
            ls >> range >> text >> regex >> needles >> wide_rows;
            bsh_rtg::Mix m;
            m.range = range != 0; m.text = text != 0;
            const char *name = bsh_rtg::wide_group_call_name(m, regex != 0, needles != 0, wide_rows != 0);
            out << (name ? name : "-") << "\n";
        } else if (kind == "F") {
            int mix_ok = 0;
            ls >> mix_ok;
            bsh_rtg::Group g;
            std::string q;
            bool first = true;
            while (ls >> q) {
                const bsh_rtg::Fresh f = fresh_of(q);
                const bool ok = bsh_rtg::wide_fits(mix_ok != 0, g, f);
                if (ok) bsh_rtg::add(g, f);
                out << (first ? "" : " ") << (ok ? 1 : 0);
                first = false;
            }
            out << "\n";
        } else {
            std::fprintf(stderr, "unknown case %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
