// Host driver of the probe plan (bloomsearch_amd/csrc/host/probe_plan.hpp — the code probe_arenas and query_solo plan and merge by),
// built with plain g++ by tests/test_probe_plan.py.  Input file: little-endian u64 words, case after case, the first word of a case
// its kind; output file: u64 words, the answers in the same order (layouts beside each case below).  `probe_plan_check bmi2` alone
// prints 1 when the CPU has BMI2 (the pdep body can run), else 0.
#include "host/probe_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <string_view>

namespace {

FILE *in = nullptr, *out = nullptr;

uint64_t get()
{
    uint64_t v = 0;
    if (fread(&v, 8, 1, in) != 1) exit(3);
    return v;
}

std::vector<uint32_t> get_u32s(uint64_t n)
{
    std::vector<uint32_t> v(n);
    for (auto &x : v) x = (uint32_t)get();
    return v;
}

std::vector<uint64_t> get_u64s(uint64_t n)
{
    std::vector<uint64_t> v(n);
    for (auto &x : v) x = get();
    return v;
}

struct At {                      // a list of block counts as the header takes it: i -> blocks
    const std::vector<uint32_t> &v;
    uint32_t operator()(uint32_t i) const { return v[i]; }
};

void put(uint64_t v) { if (fwrite(&v, 8, 1, out) != 1) exit(3); }
void put_all(const std::vector<uint64_t> &v) { for (uint64_t x : v) put(x); }

// in : n_queries Wt limit budget several_devices n_arenas local[n_arenas] global[n_arenas]
// out: survivor offsets [n_arenas + 1]; n_groups; per group n_members members... v_words out_words max_blocks max_G total_G; goff [n_groups + 1]
void plan_case()
{
    const uint32_t n_queries = (uint32_t)get(), Wt = (uint32_t)get(), limit = (uint32_t)get();
    const uint64_t budget = get();
    const bool several = get() != 0;
    const uint32_t n_arenas = (uint32_t)get();
    const std::vector<uint32_t> local = get_u32s(n_arenas), global = get_u32s(n_arenas);
    const std::vector<uint64_t> off = bsh::survivor_offsets(n_arenas, n_queries, At{global});
    put_all(off);
    const std::vector<bsh::GroupPlan> groups = bsh::plan_groups(n_arenas, At{local}, n_queries, Wt, limit, budget);
    put(groups.size());
    for (const bsh::GroupPlan &g : groups) {
        put(g.index.size());
        for (uint32_t i : g.index) put(i);
        put(g.v_words); put(g.out_words); put(g.max_blocks); put(g.max_G); put(g.total_G);
    }
    put_all(bsh::group_offsets(groups, several ? nullptr : off.data()));
}

// in : n_shards pct max_group_arenas      out: n0
void split_case()
{
    const uint64_t n = get(), pct = get(), cap = get();
    put(bsh::tail_split_cut((size_t)n, (uint32_t)pct, (size_t)cap));
}

// in : nd n_arenas n_queries local[nd][n_arenas]      out: row_base [nd + 1]; arena_off [nd][n_arenas]
void rows_case()
{
    const uint32_t nd = (uint32_t)get(), n_arenas = (uint32_t)get(), n_queries = (uint32_t)get();
    std::vector<std::vector<uint32_t>> local(nd);
    for (auto &l : local) l = get_u32s(n_arenas);
    const bsh::RowsLayout L = bsh::rows_layout(nd, n_arenas, n_queries, [&local](uint32_t d, uint32_t i) { return local[d][i]; });
    if (L.nd != nd || L.n_arenas != n_arenas || L.n_queries != n_queries) exit(4);
    put_all(L.row_base);
    for (const auto &a : L.arena_off) put_all(a);
}

// in : body (0 loop, 1 pdep, 2 the dispatching interleave_shard) Q n_local di nd Gglobal part[Q * ceil(n_local / 64)] dst[Q * Gglobal]
// out: dst afterwards
void interleave_case()
{
    const uint64_t body = get();
    const uint32_t Q = (uint32_t)get(), n_local = (uint32_t)get(), di = (uint32_t)get(), nd = (uint32_t)get();
    const uint64_t Gg = get();
    const std::vector<uint64_t> part = get_u64s((uint64_t)Q * bsh::words64(n_local));
    std::vector<uint64_t> dst = get_u64s(Q * Gg);
    if (body == 0) bsh::interleave_shard_loop(part.data(), Q, n_local, di, nd, dst.data(), Gg);
    else if (body == 1) bsh::interleave_shard_pdep(part.data(), Q, n_local, di, nd, dst.data(), Gg);
    else bsh::interleave_shard(part.data(), Q, n_local, di, nd, dst.data(), Gg);
    put_all(dst);
}

// in : Q di nd n_arenas local[n_arenas] global[n_arenas] part[sum Q * ceil(local / 64)]
// out: the zeroed layout after merge_device_part; the same after one interleave_shard call per non-empty shard
void merge_case()
{
    const uint32_t Q = (uint32_t)get(), di = (uint32_t)get(), nd = (uint32_t)get(), n_arenas = (uint32_t)get();
    const std::vector<uint32_t> local = get_u32s(n_arenas), global = get_u32s(n_arenas);
    uint64_t n_part = 0;
    for (uint32_t l : local) n_part += (uint64_t)Q * bsh::words64(l);
    const std::vector<uint64_t> part = get_u64s(n_part);
    const std::vector<uint64_t> off = bsh::survivor_offsets(n_arenas, Q, At{global});
    std::vector<uint64_t> a(off[n_arenas], 0), b(off[n_arenas], 0);
    bsh::merge_device_part(part.data(), n_arenas, At{local}, At{global}, Q, di, nd, a.data(), off.data());
    uint64_t o = 0;
    for (uint32_t i = 0; i < n_arenas; ++i) {
        if (local[i] == 0) continue;
        bsh::interleave_shard(part.data() + o, Q, local[i], di, nd, b.data() + off[i], bsh::words64(global[i]));
        o += (uint64_t)Q * bsh::words64(local[i]);
    }
    put_all(a);
    put_all(b);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && std::string_view(argv[1]) == "bmi2") { printf("%d\n", __builtin_cpu_supports("bmi2") ? 1 : 0); return 0; }
    if (argc != 3) return 2;
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const uint64_t n_cases = get();
    for (uint64_t i = 0; i < n_cases; ++i) {
        switch (get()) {
        case 0: plan_case(); break;
        case 1: split_case(); break;
        case 2: rows_case(); break;
        case 3: interleave_case(); break;
        case 4: merge_case(); break;
        default: return 2;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
