// substring_groups_check.cpp — runs bloomsearch_amd/csrc/host/substring_groups.hpp on the CPU for tests/test_substring_groups.py.
//   substring_groups_check <cases.txt> <answers.txt>
// One case per line, one answer line per case:
//   C                                               -> the four regex-table caps: batched, batched beside needles, wide, wide beside needles
//   P <len>...                                      -> per prefix of the needle lengths, added one query (= one needle) at a time:
//                                                      1 = fits() says the needle still packs, 0 = it does not (the group then stays as it was)
//   G <wide> <n_queries> (<rx_bytes> <n_needles> <len>*)*   -> per query: 1 = fits() took it into the ONE group (then add()), 0 = refused (left out)
//   K <regex> <needles> <wide> <wide_rows>          -> the name of the call group_call chooses
//   N <len>...                                      -> 1 = pack_needles (substring_pack.hpp) packs needles of these lengths, in order; else 0
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/substring_groups.hpp"

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
        if (kind == "C") {
            out << bsh_subg::regex_table_cap(false, false) << " " << bsh_subg::regex_table_cap(false, true) << " " << bsh_subg::regex_table_cap(true, false) << " "
                << bsh_subg::regex_table_cap(true, true) << "\n";
        } else if (kind == "P") {
            bsh_subg::Group g;
            uint32_t n = 0;
            bool first = true;
            while (ls >> n) {
                bsh_subg::Fresh f;
                f.needle_len.push_back(n);
                const bool ok = bsh_subg::fits(g, f, false);
                if (ok) bsh_subg::add(g, f);
                out << (first ? "" : " ") << (ok ? 1 : 0);
                first = false;
            }
            out << "\n";
        } else if (kind == "G") {
            uint32_t wide = 0, nq = 0;
            ls >> wide >> nq;
            bsh_subg::Group g;
            for (uint32_t q = 0; q < nq; ++q) {
                bsh_subg::Fresh f;
                uint32_t nn = 0;
                ls >> f.rx_bytes >> nn;
                f.needle_len.resize(nn);
                for (uint32_t &v : f.needle_len) ls >> v;
                const bool ok = bsh_subg::fits(g, f, wide != 0);
                if (ok) bsh_subg::add(g, f);
                out << (q ? " " : "") << (ok ? 1 : 0);
            }
            out << "\n";
        } else if (kind == "K") {
            uint32_t regex = 0, needles = 0, wide = 0, wide_rows = 0;
            ls >> regex >> needles >> wide >> wide_rows;
            out << bsh_subg::call_name(bsh_subg::group_call(regex != 0, needles != 0, wide != 0, wide_rows != 0)) << "\n";
        } else if (kind == "N") {
            std::vector<std::string> folded;
            std::vector<uint8_t> any_field;
            uint32_t n = 0;
            while (ls >> n) { folded.emplace_back(n, 'a'); any_field.push_back(1); }
            bsh::NeedlePack pack;
            out << (bsh::pack_needles(folded, any_field, pack) ? 1 : 0) << "\n";
        } else {
            std::fprintf(stderr, "unknown case %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
