// gather_pad_check — bsh::gather_lds_pad (bloomsearch_amd/csrc/host/probe_plan.hpp) on the CPU, driven by tests/test_gather_pad.py.
//   gather_pad_check answers.bin n
// answers.bin: the u64 words  pad(0) .. pad(n) , then kCuLdsBytes kLdsAllocUnit kLdsOptInBytes kGatherPadMax kGatherMaxWorkgroupsPerCu
// kGatherWorkgroupsPerCu.
// Plain host C++: builds with -fsanitize=address,undefined.
#include "host/probe_plan.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s answers.bin n\n", argv[0]); return 2; }
    const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10);
    std::vector<uint64_t> out;
    for (uint32_t w = 0; w <= n; ++w) {
        if (bsh::gather_lds_pad(w) != bsh::gather_lds_pad(w)) { fprintf(stderr, "%u: two calls differ\n", w); return 1; }
        out.push_back(bsh::gather_lds_pad(w));
    }
    out.push_back(bsh::kCuLdsBytes);
    out.push_back(bsh::kLdsAllocUnit);
    out.push_back(bsh::kLdsOptInBytes);
    out.push_back(bsh::kGatherPadMax);
    out.push_back(bsh::kGatherMaxWorkgroupsPerCu);
    out.push_back(bsh::kGatherWorkgroupsPerCu);
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
    fclose(f);
    return 0;
}
