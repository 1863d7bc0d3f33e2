// partition_scan_check.cpp — the keyed ingest's per-row functions on the CPU, for the sanitizer build of tests/test_partition_sanitizers.py:
// the DEVICE scanner (csrc/partition.hip.h partition_scan_row and its hash, the same source the kernels inline) and the host's
// partition_key (csrc/host/partition.hpp, what bsh_partition_key calls).
//   partition_scan_check FILE: every line of FILE is "<hex of the field name> <hex of the row>" ("-" = empty).  The row is laid into a
//   heap buffer exactly as large as the kernels may read — the aligned 8-byte words that hold it plus one word of look-ahead — at each
//   of the eight alignments, between bytes that would change the result if they were interpreted.  Prints per line
//   "<U | D:hex of the device's text | ?> <H:hex of the host's text | !>" after checking that all eight alignments agree (text and tag).
//   Then every row is scanned, hashed and host-parsed truncated at every byte (a clean run is all that is asked of those).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/partition.hpp"
#include "partition.hip.h"

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
static std::string hex(const std::string &s)
{
    static const char *d = "0123456789abcdef";
    std::string out;
    for (unsigned char c : s) { out.push_back(d[c >> 4]); out.push_back(d[c & 15]); }
    return out.empty() ? "-" : out;
}

static std::string scan(const std::string &row, size_t lead, const std::string &name)
{
    const size_t n_words = row.empty() ? 2 : ((lead + row.size() - 1) >> 3) + 2;
    std::vector<uint64_t> words(n_words);                              // a heap block of exactly the readable words
    std::string bytes(n_words * 8, ' ');
    const std::string hostile = "\"" + name + "\":\"x\\\",";
    for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = hostile[i % hostile.size()];
    memcpy(&bytes[lead], row.data(), row.size());
    memcpy(words.data(), bytes.data(), bytes.size());
    std::vector<uint8_t> nm(name.begin(), name.end());                 // a heap block of exactly the name
    const bsg::PkeyScan sc = bsg::partition_scan_row(words.data(), lead, lead + row.size(), nm.data(), (uint32_t)nm.size());
    if (sc.undecided) return "U";
    if (sc.pos < lead || sc.pos + sc.len > lead + row.size()) return "?";       // the text lies inside the row
    const std::string text(reinterpret_cast<const char *>(words.data()) + sc.pos, sc.len);
    const uint32_t tag = bsg::partition_tag_bytes(reinterpret_cast<const uint8_t *>(text.data()), sc.len, 0xFFFFFFFFu);
    const uint32_t tag2 = bsg::partition_tag_bytes(reinterpret_cast<const uint8_t *>(text.data()), sc.len, 3u);
    if (!(tag & 0x80000000u) || (tag2 & 0x7FFFFFFCu)) return "?";
    return "D:" + hex(text);
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
        std::string nh, rh, name, row;
        if (!(ls >> nh >> rh) || !unhex(nh, name) || !unhex(rh, row) || name.empty() || name.size() > bsg::kPkeyMaxName) { std::cout << "?\n"; continue; }
        const std::string got = scan(row, 0, name);
        for (size_t lead = 1; lead < 8; ++lead)
            if (scan(row, lead, name) != got) { std::cout << "alignment " << lead << " differs: " << line << "\n"; return 3; }
        std::string text;
        const bool ok = bsh::partition_key(std::string(row), name, text);   // (a heap copy of exactly the row)
        std::cout << got << " " << (ok ? "H:" + hex(text) : std::string("!")) << "\n";
        for (size_t cut = 0; cut < row.size(); ++cut) {
            scan(row.substr(0, cut), cut % 8, name);
            std::string t;
            bsh::partition_key(row.substr(0, cut), name, t);
            ++truncated;
        }
    }
    std::cout << "done " << truncated << "\n";
    return 0;
}
