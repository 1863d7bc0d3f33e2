// hist.hip.h — per-pair hit counts bucketed by a number field (bsg_match_rows_wide_hist), gfx950.
//
// Contract (include/bloomgpu.h "Bucketed hit counts"): the field names a TOP-LEVEL key by the rule of the per-set MinMax
// indexes (minmax.hip.h: byte for byte, the value itself a JSON number, the last member with the key counts) and a row's value is the
// `min` half of that contract, t = clamp(floor(v)) in int64.  With d = (uint64)t - (uint64)origin and q = d / width the row's slot is
// `below` (t < origin), bucket q (q < n_buckets) or `above`; a row without such a member is `missing`.
//
// k_bucket_rows / k_bucket_rows_sets are a scanner of their own beside the storing walker, launched once per upload chunk (the MinMax
// scanner's placement: no walker gains a register).  One lane scans one row with minmax_scan_row over ONE field — the name and the
// lane's two staging slots sit in LDS — and hist_bucket_code turns (have, st, st_min) into the row's u16 code: the bucket number or one
// of four reserved codes.  A row the scanner does not decide (an exponent literal on the field, a backslash in any top-level key) gets
// the undecided code and goes to a list of the scanner's own; the host decides its match and its bucket (bsh_hist_row).  The _sets
// instance finds the row's set and scans only rows of a set with at least one pair: the others are never walked, so never counted.
// One 64-bit division per row, none in a loop.
//
// k_pair_hist runs behind k_eval_row_programs over the part's result words and the codes.  Wave w of the grid takes pair
// w / spans_max over tiles [span * span_tiles, ...) of the pair's bit row: 16 words at a time, four lanes per word, each lane walking
// the set bits of its 16 with ctz (answers are sparse) and adding 1 per bit into the wave's LDS histogram of kHistLdsSlots u32
// (ds_add_u32; four waves: 16 432 bytes).  A pair whose tiles fit one span is written out with plain coalesced stores, zeros included;
// a pair over several spans adds its non-zero slots with global atomics into counters the call zeroed first.  Integer adds: the result
// does not depend on the order.  An undecided code is skipped (its row is in the list).  Bits past a set's last row are 0 by the
// evaluator's contract, so no code is read behind the part's rows, and a set bit means "walked and decided", so its code was written.
//
// hist_bucket_code and hist_code_slot are plain C++ shared by host and device: tests/hist_scan_check.cpp runs minmax_scan_row plus
// these very lines on the CPU under the sanitizers.
#pragma once
#include "minmax.hip.h"
#ifdef __HIPCC__
#include "match.hip.h"      // PairSetDesc, pair_set_of
#endif

namespace bsg {

constexpr uint32_t kHistMaxBuckets = 1024;      // bloomgpu.h BSG_HIST_MAX_BUCKETS
constexpr uint32_t kHistLdsSlots = kHistMaxBuckets + 3u;   // BSG_HIST_SLOTS(1024): buckets, below, above, missing
constexpr uint16_t kHistBelow = 0xFFFCu, kHistAbove = 0xFFFDu, kHistMissing = 0xFFFEu, kHistUndecided = 0xFFFFu;
constexpr uint32_t kHistSlotNone = 0xFFFFFFFFu;

// the row's code from what minmax_scan_row left for field 0: st (MM_UNDECIDED), have (bit 0) and the staged min
BSG_MM_HD uint16_t hist_bucket_code(uint32_t have, uint32_t st, long long st_min, long long origin, uint64_t width, uint32_t n_buckets)
{
    if (st & MM_UNDECIDED) return kHistUndecided;
    if (!(have & 1u)) return kHistMissing;
    if (st_min < origin) return kHistBelow;
    const uint64_t d = (uint64_t)st_min - (uint64_t)origin;      // t >= origin: the difference fits 64 bits, whatever the signs
    const uint64_t q = d / width;                                // width >= 1 (the call refuses 0)
    return q >= (uint64_t)n_buckets ? kHistAbove : (uint16_t)q;  // n_buckets <= 1024: a bucket never reaches the reserved codes
}

// a code's slot among the pair's n_buckets + 3; kHistSlotNone for the undecided code (and anything no scanner writes)
BSG_MM_HD uint32_t hist_code_slot(uint32_t code, uint32_t n_buckets)
{
    if (code < n_buckets) return code;
    if (code >= kHistBelow && code <= kHistMissing) return n_buckets + (code - kHistBelow);
    return kHistSlotNone;
}

#ifdef __HIPCC__
constexpr int kBucketThreads = 256;
constexpr uint32_t kPairHistThreads = 256;      // four waves, a (pair, span) each
constexpr uint32_t kPairHistStep = 16;          // tiles a wave takes at a time: four lanes per word
constexpr uint32_t kPairHistLdsBytes = (kPairHistThreads / 64u) * kHistLdsSlots * 4u;
static_assert(kPairHistLdsBytes == 16432u, "bloomgpu.h states k_pair_hist's LDS");

struct HistField {                              // by value in the kernel arguments
    uint8_t name[kMinMaxMaxName];
    uint32_t len;                               // 1 .. kMinMaxMaxName
};

struct BucketArgs {
    const uint8_t *rows;                        // as MatchArgs: 8-byte aligned, >= 16 readable bytes behind the last row
    const uint64_t *row_off;                    // [part rows + 1]
    const uint32_t *set_first_row;              // [n_sets + 1] in part rows      (k_bucket_rows_sets)
    const uint32_t *set_pair_off;               // [n_sets + 1]: an empty range = the set's rows are not scanned
    uint16_t *code;                             // [part rows]
    uint32_t *fallback_rows;                    // the scanner's own list (part rows)
    uint32_t *n_fallback;
    long long origin;
    uint64_t width;
    uint32_t n_buckets, n_sets;
    uint32_t row_first, row_end;                // the chunk
    uint32_t rows_per_wave;                     // multiple of 64
};

template <bool SETS>
__device__ __forceinline__ void bucket_rows_body(const BucketArgs &a, const HistField &f)
{
    __shared__ __attribute__((aligned(16))) long long st_min[kBucketThreads];
    __shared__ __attribute__((aligned(16))) long long st_max[kBucketThreads];
    __shared__ uint8_t names[kMinMaxMaxName];
    __shared__ uint8_t lens[4];
    if (threadIdx.x < kMinMaxMaxName) names[threadIdx.x] = f.name[threadIdx.x];
    if (threadIdx.x == 0) lens[0] = (uint8_t)f.len;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBucketThreads / 64) + (threadIdx.x >> 6);
    const uint64_t run_begin = a.row_first + wave * a.rows_per_wave;
    const uint32_t run_end = (uint32_t)(run_begin + a.rows_per_wave < a.row_end ? run_begin + a.rows_per_wave : a.row_end);
    const uint64_t *chunks = reinterpret_cast<const uint64_t *>(a.rows);
    for (uint64_t tile = run_begin; tile < run_end; tile += 64) {
        const uint32_t r = (uint32_t)tile + lane;
        bool live = r < run_end;
        if constexpr (SETS) {
            uint32_t set = 0, hi = a.n_sets;    // last s with set_first_row[s] <= r, as the walkers
            while (live && hi - set > 1) {
                const uint32_t mid = (set + hi) >> 1;
                if (a.set_first_row[mid] <= r) set = mid; else hi = mid;
            }
            live = live && a.set_pair_off[set + 1] > a.set_pair_off[set];
        }
        const uint64_t pos = live ? a.row_off[r] : 0;
        const uint64_t end = live ? a.row_off[r + 1] : 0;
        const MinMaxScan sc = minmax_scan_row(chunks, pos, end, names, lens, 1u, st_min + threadIdx.x, st_max + threadIdx.x, (uint32_t)kBucketThreads);
        if (!live) continue;
        const uint16_t code = hist_bucket_code(sc.have, sc.st, (sc.have & 1u) ? st_min[threadIdx.x] : 0, a.origin, a.width, a.n_buckets);
        a.code[r] = code;
        if (code == kHistUndecided) {
            const uint32_t slot = __hip_atomic_fetch_add(a.n_fallback, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.fallback_rows[slot] = r;          // each row is scanned once: at most part rows entries
        }
    }
}

__global__ __launch_bounds__(kBucketThreads) void k_bucket_rows(const BucketArgs a, const HistField f) { bucket_rows_body<false>(a, f); }
__global__ __launch_bounds__(kBucketThreads) void k_bucket_rows_sets(const BucketArgs a, const HistField f) { bucket_rows_body<true>(a, f); }

struct PairHistArgs {
    const PairSetDesc *sets;                    // [n_sets + 1], as the list passes
    const uint32_t *set_first_row;              // [n_sets + 1] in part rows
    const uint64_t *words;                      // the part's result words
    const uint16_t *code;                       // [part rows]
    uint32_t *counts;                           // [n_pairs * (n_buckets + 3)], zeroed before the launch
    uint32_t n_pairs, n_sets, n_buckets;
    uint32_t span_tiles;                        // tiles of one wave: a multiple of kPairHistStep
    uint32_t spans_max;                         // ceil(the part's largest set with a pair, in tiles / span_tiles) >= 1
};

__global__ __launch_bounds__(kPairHistThreads) void k_pair_hist(const PairHistArgs a)
{
    __shared__ uint32_t hist[kPairHistThreads / 64u][kHistLdsSlots];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t slots = a.n_buckets + 3u;    // <= kHistLdsSlots: the call refuses more buckets
    uint32_t *h = hist[wv];
    for (uint32_t i = lane; i < slots; i += 64u) h[i] = 0u;
    const uint64_t w = (uint64_t)blockIdx.x * (kPairHistThreads / 64u) + wv;
    const uint64_t lp64 = w / a.spans_max;
    const uint32_t span = (uint32_t)(w % a.spans_max);
    bool active = lp64 < a.n_pairs;
    const uint32_t lp = active ? (uint32_t)lp64 : 0u;
    const uint32_t ls = pair_set_of(a.sets, a.n_sets, lp);
    const PairSetDesc sd = a.sets[ls];
    const uint32_t T = (sd.rows + 63u) / 64u;
    const uint64_t t0 = (uint64_t)span * a.span_tiles;
    active = active && t0 < T;
    const uint32_t t1 = (uint32_t)(t0 + a.span_tiles < T ? t0 + a.span_tiles : T);
    __syncthreads();
    if (active) {
        const uint64_t *wbase = a.words + sd.word0 + (uint64_t)(lp - sd.pair0) * T;
        const uint32_t first = a.set_first_row[ls], quarter = lane & 3u;
        for (uint32_t tb = (uint32_t)t0; tb < t1; tb += kPairHistStep) {
            const uint32_t t = tb + (lane >> 2);
            if (t >= t1) continue;
            uint32_t bits = (uint32_t)(wbase[t] >> (quarter * 16u)) & 0xFFFFu;
            const uint32_t row0 = first + t * 64u + quarter * 16u;
            while (bits) {
                const uint32_t b = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t slot = hist_code_slot(a.code[row0 + b], a.n_buckets);
                if (slot < slots) __hip_atomic_fetch_add(&h[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    if (!active) return;
    uint32_t *out = a.counts + (uint64_t)lp * slots;
    if (T <= a.span_tiles) {                    // the pair is this wave's alone
        for (uint32_t i = lane; i < slots; i += 64u) out[i] = h[i];
    } else {
        for (uint32_t i = lane; i < slots; i += 64u) {
            const uint32_t v = h[i];
            if (v) __hip_atomic_fetch_add(&out[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#endif  // __HIPCC__

}  // namespace bsg
