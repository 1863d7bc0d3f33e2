// minmax_check.cpp — host/minmax.hpp on its own, for the sanitizer build of tests/test_minmax_sanitizers.py.
//   minmax_check FILE: every line of FILE is "<hex of the field names, joined by 00> <hex of the row>"; prints per line the index
//   minmax_row folds into an absent one, as "field:min:max" joined by spaces ("-" for an absent field), or "!" when the row is no JSON
//   object.  Then every row is scanned again truncated at every byte (a clean run is all that is asked of those), every index is put
//   through every operator of minmax_eval, and a prefilter tree over the fields is parsed and evaluated, so every code path of the
//   header runs under the sanitizers.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "host/minmax.hpp"

static bool unhex(const std::string &h, std::string &out)
{
    out.clear();
    if (h == "-") return true;
    if (h.size() % 2) return false;
    for (size_t i = 0; i < h.size(); i += 2) {
        const int a = bsh::JScanner::hexval(h[i]), b = bsh::JScanner::hexval(h[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((char)(a * 16 + b));
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    uint64_t truncated_ok = 0, evals = 0, passes = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fh, rh, packed, row, why;
        if (!(ls >> fh >> rh) || !unhex(fh, packed) || !unhex(rh, row)) { std::cout << "?\n"; continue; }
        std::vector<std::string> fields;
        size_t at = 0;
        for (;;) {
            const size_t z = packed.find('\0', at);
            fields.push_back(packed.substr(at, z == std::string::npos ? std::string::npos : z - at));
            if (z == std::string::npos) break;
            at = z + 1;
        }
        if (!bsh::MinMaxFieldNames::check(fields, why)) { std::cout << "?" << why << "\n"; continue; }
        std::vector<bsg_minmax> idx(fields.size(), bsg_minmax{});
        if (!bsh::minmax_row(row, fields, idx.data())) std::cout << "!\n";
        else {
            std::map<std::string, bsg_minmax> have;
            for (size_t f = 0; f < fields.size(); ++f) {
                if (f) std::cout << " ";
                if (!idx[f].present) { std::cout << "-"; continue; }
                std::cout << f << ":" << idx[f].min << ":" << idx[f].max;
                have[fields[f]] = idx[f];
                const int64_t vals[3] = {idx[f].min, 0, INT64_MAX};
                for (uint32_t op = 0; op <= bsh::MM_OP_COUNT; ++op) { evals += bsh::minmax_eval(idx[f].min, idx[f].max, op, idx[f].max, vals, 3, INT64_MIN, idx[f].min); }
            }
            std::cout << "\n";
            // Or(MinMax(field 0 >= its own min), Partition(IN p)) over this block
            const std::string tree = "{\"ExpressionType\":\"OR\",\"Children\":[{\"ExpressionType\":\"CONDITION\",\"Condition\":{\"ConditionType\":\"MINMAX\","
                                     "\"MinMaxFieldName\":\"ts\",\"MinMaxCondition\":{\"Operator\":\"GTE\",\"Value\":-5}}},{\"ExpressionType\":\"CONDITION\","
                                     "\"Condition\":{\"ConditionType\":\"PARTITION\",\"PartitionCondition\":{\"Operator\":\"IN\",\"Values\":[\"p\",\"q\"]}}},"
                                     "{\"ExpressionType\":\"AND\",\"Children\":[]}]}";
            bsh::JNode n;
            bsh::PrefilterExpression e;
            if (!bsh::parse_dom(tree, n) || !bsh::prefilter_from_json(n, e)) return 3;
            passes += bsh::prefilter_eval(e, bsh::PrefilterBlock{"q", &have});
        }
        for (size_t cut = 0; cut < row.size(); ++cut) {               // a heap copy of exactly `cut` bytes: one byte too far is a report
            std::vector<bsg_minmax> t(fields.size(), bsg_minmax{});
            const std::string part(row.data(), cut);
            std::vector<char> exact(part.begin(), part.end());
            truncated_ok += bsh::minmax_row(std::string_view(exact.data(), exact.size()), fields, t.data()) ? 1 : 0;
        }
    }
    std::cout << "done " << truncated_ok << " " << evals << " " << passes << "\n";
    return 0;
}
