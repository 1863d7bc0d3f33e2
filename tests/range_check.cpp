// range_check.cpp — host/range.hpp on its own, for the sanitizer build of tests/test_range_sanitizers.py.
//   range_check FILE: every line of FILE is "<literal> <lo> <hi>", a bound being "-" (absent), "c<int64>" (closed) or "o<int64>" (open);
//   prints one character per line: the verdict of RangeRowMatcher for FieldRange("v", lo, hi) on the row {"v":<literal>} ('0' / '1'),
//   or '?' when the line does not parse.  Then the tree of all lines' conditions under one Or is matched against the last row, the
//   guard of that tree is built, and the program of the tree is emitted, so every code path of the header runs under the sanitizers.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "host/range.hpp"

static bool bound_from(const std::string &s, bool &has, bool &open, int64_t &v)
{
    if (s == "-") { has = false; return true; }
    if (s.size() < 2 || (s[0] != 'c' && s[0] != 'o')) return false;
    bsh::JNode n;
    n.type = bsh::JType::Number;
    n.text = s.substr(1);
    has = true;
    open = s[0] == 'o';
    return bsh::int64_from_json(n, v);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line, out, last_row;
    bsh::RangeExpression all;
    all.type = bsh::RegexType::Or;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string lit, lo, hi;
        bsh::RangeBounds b;
        if (!(ls >> lit >> lo >> hi) || !bound_from(lo, b.has_lo, b.lo_open, b.lo) || !bound_from(hi, b.has_hi, b.hi_open, b.hi)) { out.push_back('?'); continue; }
        const bsh::RangeExpression e = bsh::FieldRange("v", b);
        last_row = "{\"v\":" + lit + "}";
        bsh::RangeRowMatcher m(&e);
        out.push_back(m.match(last_row) ? '1' : '0');
        if (all.children.size() < 64) all.children.push_back(e);
    }
    bsh::RangeRowMatcher m(&all);
    bsh::BloomExpression guard;
    std::vector<uint32_t> kinds, prog;
    std::vector<std::string> fields, tokens;
    bsh::emit_range_program(all, kinds, fields, tokens, prog);
    std::cout << out << "\n" << (m.match(last_row) ? 1 : 0) << " " << (bsh::range_guard(&all, guard) ? guard.children.size() : 0) << " " << kinds.size() << "\n";
    return 0;
}
