// probe_chunks_check — bsh::pipeline_chunks (bloomsearch_amd/csrc/host/probe_plan.hpp) on the CPU, driven by tests/test_probe_chunks.py.
//   probe_chunks_check cases.bin answers.bin
// cases.bin: u64 count, then per case the u64 words  n_arenas n_blocks gathers identity_few n_groups other_route key ;
// answers.bin: per case the u64 words  n_chunks size_0 .. size_{n_chunks - 1} , then the four defaults
// kPipelineMinArenas kPipelineMinBlocks kPipelineChunks kPipelineLastPct.
// Plain host C++: builds with -fsanitize=address,undefined.
#include "host/probe_plan.hpp"
#include <cstdio>
#include <cstdlib>

static std::vector<uint64_t> read_words(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> w((size_t)n / 8);
    if (!w.empty() && fread(w.data(), 8, w.size(), f) != w.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return w;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin answers.bin\n", argv[0]); return 2; }
    const std::vector<uint64_t> in = read_words(argv[1]);
    if (in.empty() || in.size() != 1 + in[0] * 7) { fprintf(stderr, "malformed cases\n"); return 2; }
    std::vector<uint64_t> out;
    for (uint64_t i = 0; i < in[0]; ++i) {
        const uint64_t *c = in.data() + 1 + i * 7;
        const bsh::PipelineCase pc{c[2] != 0, c[3] != 0, (uint32_t)c[4], c[5] != 0};
        const std::vector<uint32_t> sizes = bsh::pipeline_chunks((uint32_t)c[0], c[1], pc, c[6]);
        const std::vector<uint32_t> again = bsh::pipeline_chunks((uint32_t)c[0], c[1], pc, c[6]);
        if (sizes != again) { fprintf(stderr, "case %llu: two calls differ\n", (unsigned long long)i); return 1; }
        out.push_back(sizes.size());
        for (uint32_t s : sizes) out.push_back(s);
    }
    out.push_back(bsh::kPipelineMinArenas);
    out.push_back(bsh::kPipelineMinBlocks);
    out.push_back(bsh::kPipelineChunks);
    out.push_back(bsh::kPipelineLastPct);
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    return 0;
}
