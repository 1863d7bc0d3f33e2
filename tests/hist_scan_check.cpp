// hist_scan_check.cpp — the bucket scanner's per-row lines (csrc/minmax.hip.h minmax_scan_row plus csrc/hist.hip.h hist_bucket_code and
// hist_code_slot, the same source k_bucket_rows and k_pair_hist inline) on the CPU, for the sanitizer build of tests/test_hist_sanitizers.py.
//   hist_scan_check FILE: every line of FILE is "<hex of the field name> <origin> <width> <n_buckets> <hex of the row>" ("-": an empty
//   row).  The row is laid into a heap buffer exactly as large as the kernel may read — the aligned 8-byte words that hold it plus one
//   word of look-ahead — at each of the eight alignments, between bytes that would change the result if they were interpreted; prints
//   per line "U" when the scanner does not decide the row, else the row's slot, after checking that all eight alignments agree.  Then
//   every row is scanned truncated at every byte (a clean run is all that is asked of those).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hist.hip.h"

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

struct Spec {
    uint8_t name[bsg::kMinMaxMaxName];
    uint8_t len[4];
    long long origin;
    uint64_t width;
    uint32_t n_buckets;
};

static std::string scan(const std::string &row, size_t lead, const Spec &sp)
{
    const size_t n_words = row.empty() ? 2 : ((lead + row.size() - 1) >> 3) + 2;
    std::vector<uint64_t> words(n_words);                              // a heap block of exactly the readable words
    std::string bytes(n_words * 8, ' ');
    const char *hostile = "\"ts\":9,";
    for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = hostile[i % 7];
    memcpy(&bytes[lead], row.data(), row.size());
    memcpy(words.data(), bytes.data(), bytes.size());
    long long st_min = 0, st_max = 0;                                  // the lane's two staging slots
    const bsg::MinMaxScan sc = bsg::minmax_scan_row(words.data(), lead, lead + row.size(), sp.name, sp.len, 1u, &st_min, &st_max, 1u);
    const uint16_t code = bsg::hist_bucket_code(sc.have, sc.st, (sc.have & 1u) ? st_min : 0, sp.origin, sp.width, sp.n_buckets);
    const uint32_t slot = bsg::hist_code_slot(code, sp.n_buckets);
    if (code == bsg::kHistUndecided) return slot == bsg::kHistSlotNone ? "U" : "undecided code with a slot";
    if (slot >= sp.n_buckets + 3u) return "slot out of range";
    return std::to_string(slot);
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
        std::string fh, rh, name, row;
        Spec sp{};
        if (!(ls >> fh >> sp.origin >> sp.width >> sp.n_buckets >> rh) || !unhex(fh, name) || !unhex(rh, row) || name.empty() ||
            name.size() > bsg::kMinMaxMaxName || sp.width == 0 || sp.n_buckets == 0 || sp.n_buckets > bsg::kHistMaxBuckets) {
            std::cout << "?\n";
            continue;
        }
        memcpy(sp.name, name.data(), name.size());
        sp.len[0] = (uint8_t)name.size();
        const std::string got = scan(row, 0, sp);
        for (size_t lead = 1; lead < 8; ++lead)
            if (scan(row, lead, sp) != got) { std::cout << "alignment " << lead << " differs: " << line << "\n"; return 3; }
        std::cout << got << "\n";
        for (size_t cut = 0; cut < row.size(); ++cut) { scan(row.substr(0, cut), cut % 8, sp); ++truncated; }
    }
    std::cout << "done " << truncated << "\n";
    return 0;
}
