// minmax_scan_check.cpp — the device scanner's per-row function (csrc/minmax.hip.h minmax_scan_row, the same source the kernels inline) on
// the CPU, for the sanitizer build of tests/test_minmax_sanitizers.py.
//   minmax_scan_check FILE: every line of FILE is "<hex of the field names, joined by 00> <hex of the row>".  The row is laid into a heap
//   buffer exactly as large as the kernels may read — the aligned 8-byte words that hold it plus one word of look-ahead — at each of the
//   eight alignments, between bytes that would change the result if they were interpreted; prints per line "U" when the scanner does
//   not decide the row, else "field:min:max" joined by spaces ("-" for no contribution), after checking that all eight alignments
//   agree.  Then every row is scanned truncated at every byte (a clean run is all that is asked of those).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "minmax.hip.h"

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
static bool unhex(const std::string &h, std::string &out)
{
    out.clear();
    if (h == "-") return true;
    if (h.size() % 2) return false;
    for (size_t i = 0; i < h.size(); i += 2) {
        if (hexval(h[i]) < 0 || hexval(h[i + 1]) < 0) return false;
        out.push_back((char)(hexval(h[i]) * 16 + hexval(h[i + 1])));
    }
    return true;
}

static std::string scan(const std::string &row, size_t lead, const bsg::MinMaxFields &fl)
{
    constexpr uint32_t stride = 3;
    const size_t n_words = row.empty() ? 2 : ((lead + row.size() - 1) >> 3) + 2;
    std::vector<uint64_t> words(n_words);                              // a heap block of exactly the readable words
    std::string bytes(n_words * 8, ' ');
    const char *hostile = "\"ts\":9,";
    for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = hostile[i % 7];
    memcpy(&bytes[lead], row.data(), row.size());
    memcpy(words.data(), bytes.data(), bytes.size());
    std::vector<long long> st_min(fl.n * stride, 0), st_max(fl.n * stride, 0);
    const bsg::MinMaxScan sc = bsg::minmax_scan_row(words.data(), lead, lead + row.size(), fl.name, fl.len, (1u << fl.n) - 1u, st_min.data(), st_max.data(), stride);
    if (sc.st & bsg::MM_UNDECIDED) return "U";
    std::ostringstream out;
    for (uint32_t f = 0; f < fl.n; ++f) {
        if (f) out << " ";
        if ((sc.have >> f) & 1u) out << f << ":" << st_min[f * stride] << ":" << st_max[f * stride];
        else out << "-";
    }
    return out.str();
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    uint64_t truncated = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fh, rh, packed, row;
        if (!(ls >> fh >> rh) || !unhex(fh, packed) || !unhex(rh, row)) { std::cout << "?\n"; continue; }
        bsg::MinMaxFields fl{};
        size_t at = 0;
        bool ok = true;
        for (;;) {
            const size_t z = packed.find('\0', at);
            const std::string name = packed.substr(at, z == std::string::npos ? std::string::npos : z - at);
            if (fl.n >= bsg::kMinMaxMaxFields || name.empty() || name.size() > bsg::kMinMaxMaxName) { ok = false; break; }
            memcpy(fl.name + fl.n * bsg::kMinMaxMaxName, name.data(), name.size());
            fl.len[fl.n++] = (uint8_t)name.size();
            if (z == std::string::npos) break;
            at = z + 1;
        }
        if (!ok) { std::cout << "?\n"; continue; }
        const std::string got = scan(row, 0, fl);
        for (size_t lead = 1; lead < 8; ++lead)
            if (scan(row, lead, fl) != got) { std::cout << "alignment " << lead << " differs: " << line << "\n"; return 3; }
        std::cout << got << "\n";
        for (size_t cut = 0; cut < row.size(); ++cut) { scan(row.substr(0, cut), cut % 8, fl); ++truncated; }
    }
    std::cout << "done " << truncated << "\n";
    return 0;
}
