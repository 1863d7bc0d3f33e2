// probe_route_check.cpp — drives bsh::launch_gathers (bloomsearch_amd/csrc/host/probe_plan.hpp: does a few-term probe launch gather
// or stream) on the CPU for tests/test_probe_route.py.  Input: a file of little-endian u64 words, [n_cases] then per case
// [n_kinds, n_blocks, many_terms, gather_cost, then per kind sum_words, unstaged_words, terms, max_k]; output: two u64 per case, 1 = the launch gathers, and the sum over the kinds of bsh::gathered_bytes.
// Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/probe_plan.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin answers.bin\n", argv[0]); return 2; }
    std::vector<uint64_t> w;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint64_t v;
        while (fread(&v, 8, 1, f) == 1) w.push_back(v);
        fclose(f);
    }
    size_t at = 0;
    auto take = [&]() -> uint64_t {
        if (at >= w.size()) { fprintf(stderr, "case file ends early at word %zu\n", at); exit(2); }
        return w[at++];
    };
    std::vector<uint64_t> out;
    const uint64_t n_cases = take();
    for (uint64_t c = 0; c < n_cases; ++c) {
        const uint32_t n_kinds = (uint32_t)take();
        const uint64_t n_blocks = take();
        const bool many_terms = take() != 0;
        const uint32_t cost = (uint32_t)take();
        if (n_kinds > 3) { fprintf(stderr, "case %llu: %u kinds\n", (unsigned long long)c, n_kinds); return 2; }
        bsh::GatherKind k[3] = {};
        for (uint32_t y = 0; y < n_kinds; ++y) {
            k[y].sum_words = take();
            k[y].unstaged_words = take();
            k[y].terms = (uint32_t)take();
            k[y].max_k = (uint32_t)take();
        }
        out.push_back(bsh::launch_gathers(k, n_kinds, n_blocks, many_terms, cost) ? 1 : 0);
        uint64_t bytes = 0;
        for (uint32_t y = 0; y < n_kinds; ++y) bytes += bsh::gathered_bytes(k[y], n_blocks);
        out.push_back(bytes);
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { perror(argv[2]); return 2; }
    fclose(f);
    return 0;
}
