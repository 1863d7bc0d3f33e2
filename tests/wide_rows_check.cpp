// wide_rows_check.cpp — drives the tagged-row-list arithmetic of bloomsearch_amd/csrc/host/wide_plan.hpp (bsg_match_rows_wide_rows) on
// the CPU for tests/test_match_wide_rows_plan.py.  Input: a file of little-endian u64 words, [n_cases] then each case beginning
// with its kind; output: a file of u64 answers.  Plain C++: builds with g++ alone (and under -fsanitize=address,undefined as it stands).
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
            for (uint64_t v : {(uint64_t)bsh_wide::kPairNone, (uint64_t)bsh_wide::kPairAll, (uint64_t)bsh_wide::kPairList, (uint64_t)bsh_wide::kPairDense,
                               (uint64_t)bsh_wide::kPairScanWidth, (uint64_t)sizeof(bsh_wide::PairSet)})
                out.push_back(v);
        } else if (kind == 1) {          // tag, header and size: c, R
            const uint64_t cnt = in.take();
            const uint32_t R = (uint32_t)in.take();
            const uint32_t hdr = bsh_wide::pair_header(cnt, R);
            out.push_back(bsh_wide::pair_tag(cnt, R));
            out.push_back(hdr);
            out.push_back(bsh_wide::pair_payload_size(hdr, R));
        } else if (kind == 2) {          // offsets from headers: n_sets, first_row, pair_off, the headers from pair_off[0] on, want_off
            const uint32_t n_sets = (uint32_t)in.take();
            const std::vector<uint32_t> first = in.take32((size_t)n_sets + 1), poff = in.take32((size_t)n_sets + 1);
            const uint32_t n_pairs = poff.back() - poff.front();
            const std::vector<uint32_t> hdr = in.take32(n_pairs);
            const bool want_off = in.take() != 0;
            std::vector<uint64_t> off((size_t)n_pairs + 1, ~0ull);
            out.push_back(bsh_wide::pair_payload_offsets(hdr.data(), first.data(), poff.data(), n_sets, want_off ? off.data() : nullptr));
            if (want_off) out.insert(out.end(), off.begin(), off.end());
        } else if (kind == 3) {          // the stitch: n_sets, set_first_row, set_query_off, n_cuts, cuts; per part its headers and payload
            const uint32_t n_sets = (uint32_t)in.take();
            const std::vector<uint32_t> first = in.take32((size_t)n_sets + 1), sqo = in.take32((size_t)n_sets + 1);
            const std::vector<uint32_t> cuts = in.take32(in.take());
            const size_t n_parts = cuts.size() - 1;
            std::vector<bsh_wide::PartSets> ps(n_parts);
            std::vector<std::vector<uint32_t>> hdrs(n_parts), payloads(n_parts);
            std::vector<bsh_wide::PartRows> parts;
            for (size_t i = 0; i < n_parts; ++i) {
                ps[i] = bsh_wide::part_sets(first.data(), sqo.data(), n_sets, cuts[i], cuts[i + 1]);
                const uint32_t n_pairs = ps[i].pair_off.back() - ps[i].pair_off.front();
                hdrs[i] = in.take32(n_pairs);
                payloads[i] = in.take32(in.take());
                // what the device's passes are given of the part
                const std::vector<bsh_wide::PairSet> sets = bsh_wide::pair_sets(ps[i]);
                out.push_back(sets.size());
                for (const bsh_wide::PairSet &s : sets)
                    for (uint64_t v : {s.word0, (uint64_t)s.pair0, (uint64_t)s.rows, (uint64_t)s.tile0}) out.push_back(v);
            }
            for (size_t i = 0; i < n_parts; ++i) {
                const uint32_t n_pairs = ps[i].pair_off.back() - ps[i].pair_off.front();
                parts.push_back(bsh_wide::PartRows{&ps[i], hdrs[i].data(), payloads[i].data(), std::vector<uint64_t>((size_t)n_pairs + 1)});
                const uint64_t len = bsh_wide::pair_payload_offsets(hdrs[i].data(), ps[i].first_row.data(), ps[i].pair_off.data(), ps[i].n(), parts.back().off.data());
                if (len != payloads[i].size()) { fprintf(stderr, "part %zu: headers say %llu u32, the case holds %zu\n", i, (unsigned long long)len, payloads[i].size()); return 2; }
            }
            std::vector<uint32_t> hdr(sqo.back(), ~0u);
            const uint64_t len = bsh_wide::stitch_headers(parts, first.data(), sqo.data(), n_sets, hdr.data());
            std::vector<uint32_t> payload(len, ~0u);
            bsh_wide::stitch_payloads(parts, first.data(), sqo.data(), n_sets, hdr.data(), payload.data());
            out.insert(out.end(), hdr.begin(), hdr.end());
            out.push_back(len);
            out.insert(out.end(), payload.begin(), payload.end());
        } else if (kind == 4) {          // pair_rows_list: hdr, set_rows, cap, have_payload, payload
            const uint32_t hdr = (uint32_t)in.take(), set_rows = (uint32_t)in.take(), cap = (uint32_t)in.take();
            const bool have = in.take() != 0;
            const std::vector<uint32_t> payload = in.take32(in.take());
            std::vector<uint32_t> rows((size_t)cap + 1, 0xFEEDu);
            uint32_t n = 0xFEEDu;
            const bsh_wide::ListStatus st = bsh_wide::pair_rows_list(hdr, have ? payload.data() : nullptr, set_rows, cap ? rows.data() : nullptr, cap, &n);
            out.push_back((uint64_t)st);
            out.push_back(n);
            out.push_back(rows[cap] == 0xFEEDu);
            if (st == bsh_wide::ListStatus::Ok) out.insert(out.end(), rows.begin(), rows.begin() + std::min(n, cap));
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
