// row_program_check.cpp — drives bloomsearch_amd/csrc/host/row_program.hpp (the row matchers' one program evaluator) on the CPU for
// tests/test_row_program.py.  Input: a file of little-endian u64 words, [n_cases] then each case; output: a file of u64 answers.
// Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
//   case   reader, n_ops, op[n_ops], n_ranges, (j0, j1)[n_ranges], n_words, flag word[n_words]
//          reader 0  TERM c reads bit c & 63 of word 0 (the walkers and k_eval_row_programs: one register word)
//          reader 1  TERM c reads bit c & 63 of word c >> 6, served a word at a time: the last word fetched is kept, across the
//                    ranges of the case (k_eval_row_programs_w)
//          -> per range its verdict; reader 1: then the number of words fetched in all
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/row_program.hpp"

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

struct WordServer {
    const std::vector<uint64_t> &words;
    uint32_t cur = ~0u;
    uint64_t sat = 0, fetched = 0;
    uint64_t operator()(uint32_t c)
    {
        if ((c >> 6) != cur) {
            cur = c >> 6;
            if (cur >= words.size()) { fprintf(stderr, "TERM %u outside the case's %zu words\n", c, words.size()); exit(2); }
            sat = words[cur];
            ++fetched;
        }
        return (sat >> (c & 63u)) & 1ULL;
    }
};

static_assert(bsh_prog::eval_program((const uint32_t *)nullptr, 5, 5, [](uint32_t) { return 0; }), "the nil program matches, at compile time too");

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
        const uint64_t reader = in.take();
        std::vector<uint32_t> prog(in.take());
        for (auto &op : prog) op = (uint32_t)in.take();
        std::vector<uint64_t> ranges(2 * in.take());
        for (auto &x : ranges) x = in.take();
        std::vector<uint64_t> words(in.take());
        for (auto &x : words) x = in.take();
        if (reader > 1 || words.empty()) { fprintf(stderr, "case %llu: reader %llu, %zu words\n", (unsigned long long)k, (unsigned long long)reader, words.size()); return 2; }
        WordServer server{words};
        for (size_t i = 0; i < ranges.size(); i += 2) {
            const uint32_t j0 = (uint32_t)ranges[i], j1 = (uint32_t)ranges[i + 1];
            if (j0 > j1 || j1 > prog.size()) { fprintf(stderr, "case %llu: range [%u, %u) of %zu ops\n", (unsigned long long)k, j0, j1, prog.size()); return 2; }
            if (reader == 0) {
                const uint64_t sat = words[0];
                out.push_back(bsh_prog::eval_program(prog.data(), j0, j1, [&](uint32_t c) { return (sat >> (c & 63u)) & 1ULL; }));
            } else {
                out.push_back(bsh_prog::eval_program(prog.data(), j0, j1, server));
            }
        }
        if (reader == 1) out.push_back(server.fetched);
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { perror("write"); return 2; }
    fclose(f);
    return 0;
}
