// lookup_plan_check.cpp — drives bloomsearch_amd/csrc/host/lookup_plan.hpp (the table arithmetic of bsg_match_rows_lookup) on the CPU
// for tests/test_match_lookup_plan.py.  Input: a file of little-endian u64 words, [n_cases] then each case beginning with its kind;
// output: a file of u64 answers.  Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
//   kind 0  strings   n, h0[n], n_queries, (key, target id or kNoString)[n_queries]
//                     -> slots, table[slots], per query find_string(key, id -> h0[id] == key && (no target || id == target))
//   kind 1  table     n_conds, (kind, field number, token number)[n_conds] (string = the number in decimal; a Token condition's field
//                     and a Field condition's token are the empty string), n_queries, (fid, tid)[n_queries]
//                     -> status, bad; Ok: n_strings, rec[], string_of[2 n_conds], canon[n_conds], n_pairs, (fid, tid, cond)[],
//                     pair slots, per query find_pair
//   kind 2  flags     n_conds, part_rows, row_base, r, cond -> flag_words, flag_index, flag_bit, flag_bytes_per_row
//   kind 3  pairs     n, (fid, tid, cond)[n] -> slots, place_pairs' table[slots] (tests/test_lookup_shapes.py: slot for slot)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/lookup_plan.hpp"

namespace {

struct In {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t take()
    {
        if (at >= w.size()) { fprintf(stderr, "case file ends early at word %zu\n", at); exit(2); }
        return w[at++];
    }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin answers.bin\n", argv[0]); return 2; }
    In in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint64_t v;
        while (fread(&v, 8, 1, f) == 1) in.w.push_back(v);
        fclose(f);
    }
    std::vector<uint64_t> out;
    const uint64_t n_cases = in.take();
    for (uint64_t k = 0; k < n_cases; ++k) {
        const uint64_t kind = in.take();
        if (kind == 0) {
            const uint32_t n = (uint32_t)in.take();
            std::vector<uint64_t> h0(n);
            for (auto &x : h0) x = in.take();
            const std::vector<uint32_t> tab = bsh_lookup::place_strings(h0.data(), n);
            out.push_back(tab.size());
            out.insert(out.end(), tab.begin(), tab.end());
            const uint64_t nq = in.take();
            for (uint64_t q = 0; q < nq; ++q) {
                const uint64_t key = in.take();
                const uint32_t target = (uint32_t)in.take();
                out.push_back(bsh_lookup::find_string(tab.data(), (uint32_t)tab.size(), key, [&](uint32_t id) {
                    return h0[id] == key && (target == bsh_lookup::kNoString || id == target);
                }));
            }
        } else if (kind == 1) {
            const uint32_t n_conds = (uint32_t)in.take();
            std::vector<uint32_t> kinds(n_conds), off{0};
            std::string bytes;
            for (uint32_t c = 0; c < n_conds; ++c) {
                kinds[c] = (uint32_t)in.take();
                const uint64_t f = in.take(), t = in.take();
                if (kinds[c] != bsh_lookup::kKindToken) bytes += std::to_string(f);
                off.push_back((uint32_t)bytes.size());
                if (kinds[c] != bsh_lookup::kKindField) bytes += std::to_string(t);
                off.push_back((uint32_t)bytes.size());
            }
            bsh_lookup::Plan pl;
            uint32_t bad = 0;
            const bsh_lookup::Status st = bsh_lookup::build_strings((const uint8_t *)bytes.data(), off.data(), kinds.data(), n_conds, pl, &bad);
            out.push_back((uint64_t)st);
            out.push_back(bad);
            const uint64_t nq = in.take();
            std::vector<uint64_t> queries(2 * nq);
            for (auto &x : queries) x = in.take();
            if (st != bsh_lookup::Status::Ok) continue;
            out.push_back(pl.n_strings());
            out.insert(out.end(), pl.rec.begin(), pl.rec.end());
            out.insert(out.end(), pl.string_of.begin(), pl.string_of.end());
            out.insert(out.end(), pl.canon.begin(), pl.canon.end());
            out.push_back(pl.pairs.size());
            for (const bsh_lookup::Pair &p : pl.pairs) { out.push_back(p.fid); out.push_back(p.tid); out.push_back(p.cond); }
            const std::vector<uint64_t> tab = bsh_lookup::place_pairs(pl.pairs);
            out.push_back(tab.size());
            for (uint64_t q = 0; q < nq; ++q)
                out.push_back(bsh_lookup::find_pair(tab.data(), (uint32_t)tab.size(), (uint32_t)queries[2 * q], (uint32_t)queries[2 * q + 1]));
        } else if (kind == 2) {
            const uint32_t n_conds = (uint32_t)in.take(), part_rows = (uint32_t)in.take(), row_base = (uint32_t)in.take(), r = (uint32_t)in.take(),
                           cond = (uint32_t)in.take();
            out.push_back(bsh_lookup::flag_words(n_conds));
            out.push_back(bsh_lookup::flag_index(cond, part_rows, row_base, r));
            out.push_back(bsh_lookup::flag_bit(cond));
            out.push_back(bsh_lookup::flag_bytes_per_row(n_conds));
        } else if (kind == 3) {
            std::vector<bsh_lookup::Pair> pairs((size_t)in.take());
            for (bsh_lookup::Pair &p : pairs) { p.fid = (uint32_t)in.take(); p.tid = (uint32_t)in.take(); p.cond = (uint32_t)in.take(); }
            const std::vector<uint64_t> tab = bsh_lookup::place_pairs(pairs);
            out.push_back(tab.size());
            out.insert(out.end(), tab.begin(), tab.end());
        } else {
            fprintf(stderr, "unknown case kind %llu\n", (unsigned long long)kind);
            return 2;
        }
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { perror("write"); return 2; }
    fclose(f);
    return 0;
}
