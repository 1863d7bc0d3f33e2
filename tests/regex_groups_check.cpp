// regex_groups_check.cpp — runs bloomsearch_amd/csrc/host/regex_groups.hpp on the CPU for tests/test_regex_groups.py.
//   regex_groups_check <cases.txt> <answers.txt>
// One case per line, strings as hex ("-" = empty), one answer line per case:
//   B <field>...                                   -> co_active_bound
//   E <states> <classes> <field_len> <many>        -> rx_table_bytes
//   D <pattern>                                    -> <ok> <states> <classes>
//   C                                              -> kMaxRegexConds kSingleLdsCap kManyLdsCap kSingleSlots kManySlots kPathCap
//   T <many> <cap> <n_conds> (<kind> <field> <pattern>)* <n_queries> (<n_ops> <op>*)*
//        -> <status> <cond> <n_rx> <blob bytes> <n_est> <estimate>* <n_conds> <user mask>* <n_rx in blob> <user mask in the blob>*
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/regex_groups.hpp"

static std::string unhex(const std::string &h)
{
    if (h == "-") return std::string();
    std::string out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::stoul(h.substr(i, 2), nullptr, 16));
    return out;
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
        if (kind == "B") {
            std::vector<std::string> fields;
            std::string h;
            while (ls >> h) fields.push_back(unhex(h));
            std::vector<std::string_view> views(fields.begin(), fields.end());
            out << bsh_rxg::co_active_bound(views) << "\n";
        } else if (kind == "E") {
            uint32_t s = 0, c = 0, f = 0, many = 0;
            ls >> s >> c >> f >> many;
            out << bsh_rxg::rx_table_bytes(s, c, f, many != 0) << "\n";
        } else if (kind == "D") {
            std::string h, err;
            ls >> h;
            bsh_rx::Dfa d;
            const bool ok = bsh_rx::compile(unhex(h), d, err);
            out << (ok ? 1 : 0) << " " << d.n_states << " " << d.n_classes << "\n";
        } else if (kind == "C") {
            out << bsh_rxg::kMaxRegexConds << " " << bsh_rxg::kSingleLdsCap << " " << bsh_rxg::kManyLdsCap << " " << bsh_rxg::kSingleSlots << " "
                << bsh_rxg::kManySlots << " " << bsh_rxg::kPathCap << "\n";
        } else if (kind == "T") {
            uint32_t many = 0, cap = 0, n_conds = 0, nq = 0;
            ls >> many >> cap >> n_conds;
            std::vector<uint32_t> kinds(n_conds), coff{0};
            std::vector<uint8_t> cbytes;
            for (uint32_t c = 0; c < n_conds; ++c) {
                std::string f, p;
                ls >> kinds[c] >> f >> p;
                for (const std::string &s : {unhex(f), unhex(p)}) { cbytes.insert(cbytes.end(), s.begin(), s.end()); coff.push_back((uint32_t)cbytes.size()); }
            }
            ls >> nq;
            std::vector<uint32_t> ops, poff{0};
            for (uint32_t q = 0; q < nq; ++q) {
                uint32_t n = 0;
                ls >> n;
                for (uint32_t i = 0; i < n; ++i) { uint32_t op = 0; ls >> op; ops.push_back(op); }
                poff.push_back((uint32_t)ops.size());
            }
            const std::vector<uint64_t> users = bsh_rxg::user_masks(ops.data(), poff.data(), nq, n_conds);
            std::vector<uint32_t> blob;
            const bsh_rxg::BlobResult r = bsh_rxg::build_blob(cbytes.data(), coff.data(), kinds.data(), n_conds, 3u, cap, many ? users.data() : nullptr, blob);
            out << (int)r.status << " " << r.cond << " " << r.n_rx << " " << blob.size() * 4 << " " << r.estimate.size();
            for (uint32_t e : r.estimate) out << " " << e;
            out << " " << users.size();
            for (uint64_t u : users) out << " " << u;
            const uint32_t in_blob = (many && !blob.empty()) ? r.n_rx : 0;
            out << " " << in_blob;
            for (uint32_t j = 0; j < in_blob; ++j) out << " " << ((uint64_t)blob[4 * r.n_rx + 2 * j] | ((uint64_t)blob[4 * r.n_rx + 2 * j + 1] << 32));
            out << "\n";
        } else if (!kind.empty()) {
            std::fprintf(stderr, "unknown case kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
