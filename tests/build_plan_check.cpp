// Host driver of the build plan (bloomsearch_amd/csrc/host/build_plan.hpp — the code bsg_arena_load, plan_arena, stream_finish and the
// two build routes lay shards out, cut parts and choose a filter's route by), built with plain g++ by tests/test_build_plan.py.
// Input file: little-endian u64 words, case after case, the first word of a case its kind; output file: u64 words, the answers in
// the same order (layouts beside each case below).
#include "host/build_plan.hpp"
#include <cstdio>
#include <cstdlib>

namespace {

FILE *in = nullptr, *out = nullptr;

uint64_t get()
{
    uint64_t v = 0;
    if (fread(&v, 8, 1, in) != 1) exit(3);
    return v;
}

void put(uint64_t v) { if (fwrite(&v, 8, 1, out) != 1) exit(3); }

void put_stats(const bsh::ShardStats &s)
{
    for (int c = 0; c < 3; ++c) put(s.sum_words[c]);
    for (int c = 0; c < 3; ++c) put(s.max_staged_words[c]);
    for (int c = 0; c < 3; ++c) put(s.fixed_m[c]);
    for (int c = 0; c < 3; ++c) put(s.fixed_k[c]);
    for (int c = 0; c < 3; ++c) put(s.geometry_uniform[c] ? 1 : 0);
}

// in : n [word_off m k] x n
std::vector<bsg_filter_desc> get_descs()
{
    std::vector<bsg_filter_desc> d(get());
    for (auto &f : d) { f.word_off = get(); f.m = get(); f.k = (uint32_t)get(); f.reserved = 0; }
    return d;
}

// in : nd descs (three per block)
// out: per device: n_local n_words; [word_off m k] x 3 n_local; per local block [block_off span_words]; the stats;
//      the stats again from add_filter over the laid-out filters alone (what stream_finish does with the decoded descriptors)
void shard_case()
{
    const uint32_t nd = (uint32_t)get();
    const std::vector<bsg_filter_desc> desc = get_descs();
    const uint32_t n_blocks = (uint32_t)(desc.size() / 3);
    for (uint32_t di = 0; di < nd; ++di) {
        const bsh::ShardLayout L = bsh::layout_shard(desc.data(), n_blocks, di, nd);
        if (L.n_blocks != bsh::shard_blocks(n_blocks, di, nd) || L.filters.size() != (size_t)L.n_blocks * 3 || L.block_off.size() != L.n_blocks) exit(4);
        put(L.n_blocks); put(L.n_words);
        for (const bsg_filter_desc &f : L.filters) { put(f.word_off); put(f.m); put(f.k); }
        for (uint32_t lb = 0; lb < L.n_blocks; ++lb) { put(L.block_off[lb]); put(bsh::block_span_words(&L.filters[(size_t)lb * 3])); }
        put_stats(L.stats);
        bsh::ShardStats fold;
        for (size_t i = 0; i < L.filters.size(); ++i) fold.add_filter((uint32_t)(i % 3), L.filters[i].m, L.filters[i].k);
        put_stats(fold);
    }
}

// in : descs n_words sections n_parts [i0 i1] x n_parts region_cap poison; with sections, per part its (i1 - i0) / 3 + 1 local offsets
// out: ascending region_bytes region_fits; [w_lo w_hi region_off region_len] x n_parts;
//      without sections: a buffer of n_words x poison after zero_unowned; with: sec_off [n_desc / 3 + 1] (poison where no part wrote)
void parts_case()
{
    const std::vector<bsg_filter_desc> desc = get_descs();
    const uint64_t n_words = get();
    const bool sections = get() != 0;
    std::vector<bsh::PartSpan> parts(get());
    for (auto &P : parts) { P.i0 = (uint32_t)get(); P.i1 = (uint32_t)get(); }
    const uint64_t cap = get(), poison = get();
    const uint64_t region_bytes = bsh::plan_parts(desc.data(), parts, n_words, sections);
    put(bsh::offsets_ascend(desc.data(), (uint32_t)desc.size()) ? 1 : 0); put(region_bytes); put(bsh::region_fits(region_bytes, cap) ? 1 : 0);
    for (const auto &P : parts) { put(P.w_lo); put(P.w_hi); put(P.region_off); put(P.region_len); }
    if (!sections) {
        std::vector<uint64_t> words(n_words, poison);
        bsh::zero_unowned(words.data(), n_words, parts);
        for (uint64_t w : words) put(w);
    } else {
        std::vector<uint64_t> sec_off(desc.size() / 3 + 1, poison);
        for (const auto &P : parts) {
            std::vector<uint64_t> local((P.i1 - P.i0) / 3 + 1);
            for (auto &x : local) x = get();
            bsh::scatter_sec_off(sec_off.data(), P, local);
        }
        for (uint64_t x : sec_off) put(x);
    }
}

// in : m n_entries k lds_head_bytes bin_min_locs bin_scratch_bytes      out: 0 staged, 1 binned, 2 sliced
void route_case()
{
    const uint64_t m = get(), n = get(), k = get(), head = get(), min_locs = get(), scratch = get();
    switch (bsh::build_route(m, n, k, (uint32_t)head, min_locs, scratch)) {
    case bsh::BuildRoute::Staged: put(0); break;
    case bsh::BuildRoute::Binned: put(1); break;
    case bsh::BuildRoute::Sliced: put(2); break;
    }
}

// in : parts unit n cost[n]      out: n_cuts cuts
void cuts_case()
{
    const uint32_t parts = (uint32_t)get(), unit = (uint32_t)get();
    std::vector<uint64_t> cost(get());
    for (auto &c : cost) c = get();
    const std::vector<uint32_t> cuts = bsh::balanced_cuts(cost, parts, unit);
    put(cuts.size());
    for (uint32_t c : cuts) put(c);
}

// out: the constants the header states
void consts_case() { put(bsh::kLdsBudget); put(bsh::kLdsCapWords); put(bsh::kAlignWords); put(bsh::kSetListBytes); }

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint64_t n_cases = get();
    for (uint64_t i = 0; i < n_cases; ++i) {
        switch (get()) {
        case 0: shard_case(); break;
        case 1: parts_case(); break;
        case 2: route_case(); break;
        case 3: cuts_case(); break;
        case 4: consts_case(); break;
        default: return 2;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
