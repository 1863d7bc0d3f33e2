// wide_plan_check.cpp — drives bloomsearch_amd/csrc/host/wide_plan.hpp (the arithmetic of the row-matcher calls) on the CPU for
// tests/test_match_wide_plan.py.  Input: a file of little-endian u64 words, [n_cases] then each case beginning with its kind;
// output: a file of u64 answers.  Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/wide_plan.hpp"

namespace {

struct In {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t take()
    {
        if (at >= w.size()) { fprintf(stderr, "case file ends early at word %zu\n", at); exit(2); }
        return w[at++];
    }
    std::vector<uint32_t> take32(size_t n)
    {
        std::vector<uint32_t> v(n);
        for (auto &x : v) x = (uint32_t)take();
        return v;
    }
    std::vector<uint64_t> take64(size_t n)
    {
        std::vector<uint64_t> v(n);
        for (auto &x : v) x = take();
        return v;
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
    for (uint64_t c = 0; c < n_cases; ++c) {
        const uint64_t kind = in.take();
        if (kind == 0) {                 // the header's constants
            for (uint64_t v : {(uint64_t)bsh_wide::kMaxQueries, (uint64_t)bsh_wide::kMaxOps, (uint64_t)bsh_wide::kMaxPairs, (uint64_t)bsh_wide::kMaxItems,
                               (uint64_t)bsh_wide::kItemPairs, (uint64_t)bsh_wide::kWideLdsCap, (uint64_t)sizeof(bsh_wide::EvalItem)})
                out.push_back(v);
        } else if (kind == 1) {          // pair_words: n_sets, n_rows, n_queries, have_first, have_off, want_offsets, the two tables
            const uint32_t n_sets = (uint32_t)in.take(), n_rows = (uint32_t)in.take(), n_queries = (uint32_t)in.take();
            const bool have_first = in.take() != 0, have_off = in.take() != 0, want_off = in.take() != 0;
            const std::vector<uint32_t> first = in.take32(have_first ? (size_t)n_sets + 1 : 0), off = in.take32(have_off ? (size_t)n_sets + 1 : 0);
            const size_t n_pairs = have_off && !off.empty() ? off.back() : n_queries;
            std::vector<uint64_t> pwo(n_pairs + 1, ~0ull);
            uint64_t total = ~0ull;
            const bsh_wide::SizeStatus st = bsh_wide::pair_words(have_first ? first.data() : nullptr, have_off ? off.data() : nullptr, n_sets, n_rows,
                                                                 n_queries, want_off ? pwo.data() : nullptr, &total);
            out.push_back((uint64_t)st);
            if (st != bsh_wide::SizeStatus::Ok) continue;
            out.push_back(total);
            out.push_back(want_off ? n_pairs + 1 : 0);
            if (want_off) out.insert(out.end(), pwo.begin(), pwo.end());
        } else if (kind == 2) {          // condition masks: n_conds, n_queries, prog_off, ops, n_sets, set_query_off, set_queries
            const uint32_t n_conds = (uint32_t)in.take(), n_queries = (uint32_t)in.take();
            const std::vector<uint32_t> poff = in.take32((size_t)n_queries + 1), ops = in.take32(poff.back());
            const uint32_t n_sets = (uint32_t)in.take();
            const std::vector<uint32_t> sqo = in.take32((size_t)n_sets + 1), sq = in.take32(sqo.back());
            const std::vector<uint64_t> qm = bsh_wide::query_cond_masks(ops.data(), poff.data(), n_queries, n_conds);
            const std::vector<uint64_t> sm = bsh_wide::set_cond_masks(qm, sqo.data(), sq.data(), n_sets);
            out.insert(out.end(), qm.begin(), qm.end());
            out.insert(out.end(), sm.begin(), sm.end());
        } else if (kind == 3) {          // parts: n_rows, row_off, n_sets, set_first_row, set_query_off, want
            const uint32_t n_rows = (uint32_t)in.take();
            const std::vector<uint64_t> row_off = in.take64((size_t)n_rows + 1);
            const uint32_t n_sets = (uint32_t)in.take();
            const std::vector<uint32_t> first = in.take32((size_t)n_sets + 1), sqo = in.take32((size_t)n_sets + 1);
            const uint32_t want = (uint32_t)in.take();
            const std::vector<uint32_t> cuts = bsh_wide::part_cuts(row_off.data(), n_rows, first.data(), n_sets, want);
            out.push_back(cuts.size());
            out.insert(out.end(), cuts.begin(), cuts.end());
            for (size_t i = 0; i + 1 < cuts.size(); ++i) {
                const bsh_wide::PartSets ps = bsh_wide::part_sets(first.data(), sqo.data(), n_sets, cuts[i], cuts[i + 1]);
                out.push_back(ps.s0);
                out.push_back(ps.n());
                out.insert(out.end(), ps.first_row.begin(), ps.first_row.end());
                out.insert(out.end(), ps.pair_off.begin(), ps.pair_off.end());
                out.insert(out.end(), ps.tile0.begin(), ps.tile0.end());
                std::vector<bsh_wide::EvalItem> items;
                uint64_t words = 0;
                const bool ok = bsh_wide::eval_items(ps, items, words);
                out.push_back(ok);
                out.push_back(words);
                out.push_back(items.size());
                for (const bsh_wide::EvalItem &it : items)
                    for (uint64_t v : {it.out0, (uint64_t)it.row0, (uint64_t)it.n_rows, (uint64_t)it.pair0, (uint64_t)it.pair1, (uint64_t)it.stride})
                        out.push_back(v);
            }
        } else if (kind == 4) {          // the single and batched calls' cuts (one implicit set of all rows): n_rows, row_off, want
            const uint32_t n_rows = (uint32_t)in.take();
            const std::vector<uint64_t> row_off = in.take64((size_t)n_rows + 1);
            const uint32_t want = (uint32_t)in.take(), all_rows[2] = {0, n_rows};
            const std::vector<uint32_t> cuts = bsh_wide::part_cuts(row_off.data(), n_rows, all_rows, 1, want);
            out.push_back(cuts.size());
            out.insert(out.end(), cuts.begin(), cuts.end());
        } else if (kind == 5) {          // a part's set range: n_sets, set_first_row, r0, r1
            const uint32_t n_sets = (uint32_t)in.take();
            const std::vector<uint32_t> first = in.take32((size_t)n_sets + 1);
            const uint32_t r0 = (uint32_t)in.take(), r1 = (uint32_t)in.take();
            const bsh_wide::SetRange sr = bsh_wide::part_set_range(first.data(), n_sets, r0, r1);
            out.push_back(sr.s0);
            out.push_back(sr.n());
            out.insert(out.end(), sr.first_row.begin(), sr.first_row.end());
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
