// ingest_plan.hpp — the arithmetic of the device ingest's host side (ingest_api.inc), free of any device type: how the slot storage
// of a run of distinct-entry tables is laid out, how many slots a table starts with and grows to, how the rows of a launch are dealt
// to waves, how fine the file-level union partitions, which of the six walkers serves a call, and what the row arguments must satisfy.
// tests/ingest_plan_check.cpp runs the same code on the CPU (tests/test_ingest_plan.py).  DESIGN.md, "Device ingest: the plan".
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace bsh {

// ---- tables: one allocation holds every table's 32-byte slots (four base hashes) first, then every table's 8-byte fingerprints ----
constexpr uint64_t kSlotBytes = 40;
constexpr uint64_t kMaxTableSlots = 1ull << 31;
constexpr uint64_t kMinTableSlots = 64;          // also the placeholder of a parent nothing inserts into before the finish step sizes it
constexpr uint64_t kGrowth = 4;

inline uint32_t pow2_at_least(uint64_t n)
{
    uint64_t c = kMinTableSlots;
    while (c < n && c < kMaxTableSlots) c <<= 1;
    return (uint32_t)c;
}

inline uint32_t shift_for(uint64_t cap)          // 32 - log2(cap) for a power-of-two capacity (IngestTable::shift)
{
    uint32_t lg = 0;
    while ((1ull << lg) < cap) ++lg;
    return 32u - lg;
}

struct TablePlace { uint64_t *slots, *fps; uint32_t mask, shift; };       // IngestTable, member for member

// Table of n slots at first_slot of a block of total_slots.  Hashed: n is a power of two and an entry's home is the top log2(n) bits
// of its key.  Dense: a list of n entries, no home (shift 0).
inline TablePlace place_table(void *base, uint64_t first_slot, uint64_t total_slots, uint64_t n, bool dense = false)
{
    uint64_t *const words = (uint64_t *)base;
    return TablePlace{words + first_slot * 4, words + total_slots * 4 + first_slot, (uint32_t)(n - 1), dense ? 0u : shift_for(n)};
}

struct TableLayout {
    std::vector<uint64_t> cap, first_slot;
    uint64_t total_slots = 0;
    bool dense = false;
    uint64_t bytes() const { return total_slots * kSlotBytes; }
    TablePlace place(void *base, size_t i) const { return place_table(base, first_slot[i], total_slots, cap[i], dense); }
};

// want[i] slots for table i: rounded to a power of two (64 at least, 2^31 at most) for hashed tables, taken as they are for dense ones
inline TableLayout layout_tables(const std::vector<uint64_t> &want, bool dense = false)
{
    TableLayout l;
    l.dense = dense;
    for (uint64_t w : want) {
        l.cap.push_back(dense ? w : pow2_at_least(w));
        l.first_slot.push_back(l.total_slots);
        l.total_slots += l.cap.back();
    }
    return l;
}

// kind 0 = the field table (fields are few), 1 / 2 = tokens / field::tokens.  A non-zero hint wins.
inline uint64_t oneshot_slots(uint32_t kind, uint64_t rows_in, uint32_t hint)      // 4 slots per row unless the caller knows better
{
    return hint ? hint : kind == 0 ? 256 : std::max<uint64_t>(1024, rows_in * 4);
}
inline uint64_t stream_slots(uint32_t kind, uint32_t hint) { return hint ? hint : kind == 0 ? 256 : 1024; }      // no row count is known when a set is made
inline uint64_t parent_slots(uint64_t child_sum) { return std::max<uint64_t>(kMinTableSlots, child_sum * 2); }   // 2 x the children bounds the union
inline uint64_t grown_slots(uint64_t cap) { return cap * kGrowth > kMaxTableSlots ? 0 : cap * kGrowth; }          // 0: refused
// descriptors / counters a streaming part makes room for: twice as many, partitions keep showing up
inline uint32_t descriptor_room(uint32_t nt) { return std::max<uint32_t>(96, nt > 0x7FFFFFFFu ? nt : nt * 2); }
// sets the MinMax records make room for; 0: room * n_fields records are more than the scanner indexes
inline uint64_t minmax_room(uint32_t n_sets, bool roomy, uint32_t n_fields)
{
    const uint64_t room = roomy ? std::max<uint64_t>(32, (uint64_t)n_sets * 2) : std::max<uint64_t>(n_sets, 1);
    return room * n_fields > 0x7FFFFFFFull ? 0 : room;
}

// ---- launches: as many waves as the device holds at once (waves_per_simd on each of a CU's 4 SIMDs), each with a contiguous run of
// rows_per_wave rows (a multiple of 64); the grid is the waves that get a row, in workgroups of `threads`.  n_rows > 0. ----
struct WaveRuns { uint32_t rows_per_wave, grid; };
inline WaveRuns wave_runs(uint64_t n_rows, uint32_t n_cus, uint32_t waves_per_simd, uint32_t threads)
{
    const uint64_t waves = std::min<uint64_t>((n_rows + 63) / 64, (uint64_t)n_cus * 4 * waves_per_simd);
    const uint64_t rpw = ((n_rows + waves - 1) / waves + 63) / 64 * 64;
    const uint64_t used = (n_rows + rpw - 1) / rpw, wpw = threads / 64;
    return WaveRuns{(uint32_t)rpw, (uint32_t)((used + wpw - 1) / wpw)};
}

// ---- the partitioned union: a parent of child_sum child entries is cut into 2^log2P partitions of about `target` entries.
// coarsen (lab): below 32 that many levels coarser (to exercise the retry and the fallback), 32 + v = 2^v x finer. ----
inline uint32_t first_log2P(uint64_t child_sum, uint32_t target, uint32_t coarsen)
{
    uint32_t lg = 0;
    while ((child_sum >> lg) > target && lg < 24) ++lg;
    return coarsen < 32 ? lg - std::min(lg, coarsen) : std::min(lg + (coarsen - 32), 24u);
}
inline uint32_t finer_log2P(uint32_t log2P) { return std::min(log2P + 2, 26u); }         // the retry: 4 x finer

// ---- walkers: (rows form) x (tokenizer) -> one of six ----
constexpr uint32_t kWalkerSlots = 6;
inline uint32_t walker_slot(bool by_set, bool spec, bool gram) { return (by_set ? 3u : 0u) + (!spec ? 0u : gram ? 2u : 1u); }

// ---- row arguments: which check fails first, and where ----
enum class RowFault : uint32_t { None, OffsetsNotMonotone, BytesMissing, SetFirstSpan, SetFirstNotMonotone, ParentsMissing, ParentOutOfRange };
struct RowCheck { RowFault fault = RowFault::None; uint32_t at = 0; };

inline RowCheck check_rows(const uint64_t *row_off, uint32_t n_rows, bool have_bytes)
{
    for (uint32_t r = 0; r < n_rows; ++r)
        if (row_off[r + 1] < row_off[r]) return {RowFault::OffsetsNotMonotone, r};
    if (row_off[n_rows] && !have_bytes) return {RowFault::BytesMissing, 0};
    return {};
}
inline RowCheck check_set_first(const uint32_t *set_first_row, uint32_t n_sets, uint32_t n_rows)
{
    if (set_first_row[0] != 0 || set_first_row[n_sets] != n_rows) return {RowFault::SetFirstSpan, 0};
    for (uint32_t s = 0; s < n_sets; ++s)
        if (set_first_row[s + 1] < set_first_row[s]) return {RowFault::SetFirstNotMonotone, s};
    return {};
}
inline RowCheck check_parents(const uint32_t *parent_of_set, uint32_t n_sets, uint32_t n_parents)      // 0xFFFFFFFF: no parent
{
    if (n_sets && n_parents && !parent_of_set) return {RowFault::ParentsMissing, 0};
    for (uint32_t s = 0; s < n_sets && parent_of_set; ++s)
        if (parent_of_set[s] != 0xFFFFFFFFu && parent_of_set[s] >= n_parents) return {RowFault::ParentOutOfRange, s};
    return {};
}
inline bool too_many_tables(uint64_t sets_and_parents) { return sets_and_parents > 0xFFFFFFFFu / 3; }      // three tables each, 32-bit indices

}  // namespace bsh
