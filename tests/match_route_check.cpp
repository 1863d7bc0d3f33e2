// match_route_check.cpp — drives bloomsearch_amd/csrc/host/match_route.hpp (which tables a row-matcher call builds, which walker
// serves it) on the CPU for tests/test_match_route.py.  Input: a text file, one case per line; output: one line per case on stdout.
//   specs                          -> one line: every CallSpec as name:mode:accepts:policy, in kCallSpecs order
//   walkers                        -> one line: every line of BSH_MATCH_WALKERS as mode:set:tok:kernel:slot
//   slots                          -> one line: kSlots, then slot(mode, set, tok) for every mode, set and tokenizer (-1: none)
//   route SPEC N_QUERIES N K0 K1.. -> status refusal cond kind blob cap users needles range consumers trace
// Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/match_route.hpp"

namespace {

using namespace bsh_route;

const char *const kModes[] = {"Single", "Many", "Wide", "Lookup"};
const char *const kSets[] = {"None", "Regex", "Substr", "RegexSubstr", "Range", "RegexSubstrRange"};
const char *const kTokNames[] = {"Default", "Spec", "Gram"};
const char *const kAccepts[] = {"Plain", "Regex", "Substr", "Range", "RegexSubstr", "All"};
const char *const kPolicies[] = {"Bits", "Rows", "Hist"};
const char *const kCaps[] = {"None", "Single", "SingleSub", "Many", "ManySub", "Wide", "WideSub", "Lookup"};
const char *const kRefusals[] = {"None", "UnknownKind", "RegexWithSubstr", "TextWithRange", "RegexInBatched"};
const char *const kStatuses[] = {"Ok", "Invalid", "Unsupported"};

struct WalkerLine {
    Mode mode;
    Consumers set;
    Tok tok;
    const char *kernel;
};
#define WALKER_LINE(M, C, T, K) {Mode::M, Consumers::C, Tok::T, #K},
const WalkerLine kWalkerLines[] = {BSH_MATCH_WALKERS(WALKER_LINE)};
#undef WALKER_LINE

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { perror(argv[1]); return 2; }
    const size_t n_specs = sizeof(kCallSpecs) / sizeof(kCallSpecs[0]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op;
        ls >> op;
        if (op == "specs") {
            for (size_t i = 0; i < n_specs; ++i) {
                const CallSpec &s = *kCallSpecs[i];
                std::cout << (i ? " " : "") << s.name << ":" << kModes[(int)s.mode] << ":" << kAccepts[(int)s.accepts] << ":" << kPolicies[(int)s.policy];
            }
            std::cout << "\n";
        } else if (op == "walkers") {
            bool first = true;
            for (const WalkerLine &w : kWalkerLines) {
                std::cout << (first ? "" : " ") << kModes[(int)w.mode] << ":" << kSets[(int)w.set] << ":" << kTokNames[(int)w.tok] << ":" << w.kernel << ":"
                          << (int32_t)slot(w.mode, w.set, w.tok);
                first = false;
            }
            std::cout << "\n";
        } else if (op == "slots") {
            std::cout << kSlots;
            for (int m = 0; m < 4; ++m)
                for (int c = 0; c < 6; ++c)
                    for (int t = 0; t < 3; ++t) std::cout << " " << (int32_t)slot((Mode)m, (Consumers)c, (Tok)t);
            std::cout << "\n";
        } else if (op == "route") {
            size_t spec = 0;
            uint32_t n_queries = 0, n = 0;
            ls >> spec >> n_queries >> n;
            if (!ls || spec >= n_specs) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
            std::vector<uint32_t> kinds(n);          // exactly n: a read past the table is the sanitizer's to find
            for (uint32_t &k : kinds) ls >> k;
            if (!ls) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
            const Route r = route(*kCallSpecs[spec], kinds.data(), n, n_queries);
            std::cout << kStatuses[(int)r.status()] << " " << kRefusals[(int)r.refusal] << " " << r.cond << " " << r.kind << " " << r.blob << " " << kCaps[(int)r.cap]
                      << " " << r.user_masks << " " << r.needles << " " << r.range_table << " " << kSets[(int)r.consumers] << " " << (r.trace ? r.trace : "-") << "\n";
        } else {
            fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
