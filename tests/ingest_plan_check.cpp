// Host driver of the device ingest's plan (bloomsearch_amd/csrc/host/ingest_plan.hpp — the arithmetic ingest_api.inc lays tables out,
// sizes launches and checks row arguments by), built with plain g++ by tests/test_ingest_plan.py, once with -Wall -Wextra -Werror and
// once under the address and undefined-behaviour sanitizers.  Input file: one command per line, a word and unsigned integers.  Output:
// one line of integers per command.
//   pow2 n                       -> capacity shift
//   oneshot kind rows_in hint    -> wanted slots, capacity          stream kind hint / parent child_sum: the same
//   grow cap                     -> the grown capacity, 0 when refused
//   room nt                      -> descriptor room                 mmroom n_sets roomy n_fields -> sets, 0 when refused
//   layout dense n want...       -> total_slots bytes, then per table: cap first_slot slots_word fps_word mask shift (words from the base)
//   place first total n dense    -> slots_word fps_word mask shift
//   wave n n_cus waves_per_simd threads -> rows_per_wave grid
//   log2p child_sum target coarsen -> log2P                         finer log2P -> log2P
//   slot by_set spec gram        -> walker slot
//   rows n have_bytes off...     -> fault index                     (n + 1 offsets)
//   setfirst n_sets n_rows v...  -> fault index                     (n_sets + 1 values)
//   parents n_sets n_parents has_array v... -> fault index
//   toomany n                    -> 0 / 1
#include "host/ingest_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

static void print_place(const bsh::TablePlace &p, const uint64_t *base)
{
    printf("%" PRIu64 " %" PRIu64 " %u %u", (uint64_t)(p.slots - base), (uint64_t)(p.fps - base), p.mask, p.shift);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    std::string text;
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    std::istringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        std::vector<uint64_t> a;
        for (uint64_t v; in >> v;) a.push_back(v);
        auto need = [&](size_t n) { return a.size() >= n; };
        auto fault = [](const bsh::RowCheck &c) { printf("%u %u\n", (uint32_t)c.fault, c.at); };
        if (cmd == "pow2" && need(1)) {
            const uint32_t cap = bsh::pow2_at_least(a[0]);
            printf("%u %u\n", cap, bsh::shift_for(cap));
        } else if (cmd == "oneshot" && need(3)) {
            const uint64_t w = bsh::oneshot_slots((uint32_t)a[0], a[1], (uint32_t)a[2]);
            printf("%" PRIu64 " %u\n", w, bsh::pow2_at_least(w));
        } else if (cmd == "stream" && need(2)) {
            const uint64_t w = bsh::stream_slots((uint32_t)a[0], (uint32_t)a[1]);
            printf("%" PRIu64 " %u\n", w, bsh::pow2_at_least(w));
        } else if (cmd == "parent" && need(1)) {
            const uint64_t w = bsh::parent_slots(a[0]);
            printf("%" PRIu64 " %u\n", w, bsh::pow2_at_least(w));
        } else if (cmd == "grow" && need(1)) {
            printf("%" PRIu64 "\n", bsh::grown_slots(a[0]));
        } else if (cmd == "room" && need(1)) {
            printf("%u\n", bsh::descriptor_room((uint32_t)a[0]));
        } else if (cmd == "mmroom" && need(3)) {
            printf("%" PRIu64 "\n", bsh::minmax_room((uint32_t)a[0], a[1] != 0, (uint32_t)a[2]));
        } else if (cmd == "layout" && need(2) && need(2 + a[1])) {
            const bsh::TableLayout l = bsh::layout_tables(std::vector<uint64_t>(a.begin() + 2, a.begin() + 2 + a[1]), a[0] != 0);
            if (l.total_slots > (1u << 22)) return 3;                           // (the cases stay small: the block below is real memory)
            std::vector<uint64_t> block(l.total_slots * 5 + 1);
            printf("%" PRIu64 " %" PRIu64, l.total_slots, l.bytes());
            for (size_t i = 0; i < l.cap.size(); ++i) {
                printf("  %" PRIu64 " %" PRIu64 " ", l.cap[i], l.first_slot[i]);
                print_place(l.place(block.data(), i), block.data());
            }
            printf("\n");
        } else if (cmd == "place" && need(4)) {
            if (a[1] > (1u << 22)) return 3;
            std::vector<uint64_t> block(a[1] * 5 + 1);
            print_place(bsh::place_table(block.data(), a[0], a[1], a[2], a[3] != 0), block.data());
            printf("\n");
        } else if (cmd == "wave" && need(4)) {
            const bsh::WaveRuns r = bsh::wave_runs(a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]);
            printf("%u %u\n", r.rows_per_wave, r.grid);
        } else if (cmd == "log2p" && need(3)) {
            printf("%u\n", bsh::first_log2P(a[0], (uint32_t)a[1], (uint32_t)a[2]));
        } else if (cmd == "finer" && need(1)) {
            printf("%u\n", bsh::finer_log2P((uint32_t)a[0]));
        } else if (cmd == "slot" && need(3)) {
            const uint32_t s = bsh::walker_slot(a[0] != 0, a[1] != 0, a[2] != 0);
            if (s >= bsh::kWalkerSlots) return 3;
            printf("%u\n", s);
        } else if (cmd == "rows" && need(2) && need(3 + a[0])) {
            const std::vector<uint64_t> off(a.begin() + 2, a.begin() + 3 + a[0]);
            fault(bsh::check_rows(off.data(), (uint32_t)a[0], a[1] != 0));
        } else if (cmd == "setfirst" && need(2) && need(3 + a[0])) {
            const std::vector<uint32_t> v(a.begin() + 2, a.begin() + 3 + a[0]);
            fault(bsh::check_set_first(v.data(), (uint32_t)a[0], (uint32_t)a[1]));
        } else if (cmd == "parents" && need(3) && need(3 + (a[2] ? a[0] : 0))) {
            const std::vector<uint32_t> v(a.begin() + 3, a.begin() + 3 + (a[2] ? a[0] : 0));
            fault(bsh::check_parents(a[2] ? v.data() : nullptr, (uint32_t)a[0], (uint32_t)a[1]));
        } else if (cmd == "toomany" && need(1)) {
            printf("%d\n", bsh::too_many_tables(a[0]) ? 1 : 0);
        } else {
            fprintf(stderr, "bad command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
