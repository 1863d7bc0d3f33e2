// minmax.hip.h — per-set MinMax indexes of a device ingest (partitionBuffer.minMaxIndexes, ingest.go:444-471), gfx950.
//
// Contract (include/bloomgpu.h): a field names a TOP-LEVEL key of the row object, compared byte for byte; the member's
// value must itself be a JSON number; of several members with the key the LAST one counts (a Go map after decoding); the number's
// exact decimal value v contributes min = clamp(floor(v)), max = clamp(ceil(v)) in int64.  A set's index for a field is the fold of
// its rows' contributions and is present only if some row contributed.
//
// k_minmax_rows / k_minmax_rows_sets are a scanner of their own, not a consumer of the ingest walker: nothing is tokenised, hashed or
// inserted, so the walkers keep their registers and their three waves per SIMD.  One lane scans one row byte by byte and tracks the
// container depth (a counter: no nesting limit), string and escape state and, at depth 1, the key: a bitmask of the fields the key
// may still be, narrowed byte by byte against the names in LDS, so "ts" is told from "t", from "tsx" and a 64-byte name from a
// 65-byte key.  A number on a matched key is parsed with NumLane's arithmetic (match.hip.h: sign, u64 magnitude with a sticky overflow
// bit, "the fraction has a non-zero digit", "has an exponent").  The row's contributions are staged per (lane, field) in LDS — a
// later member with the same key overwrites or erases the slot, which is "last wins" — and COMMITTED ONLY AFTER THE WHOLE ROW was
// scanned: a row with an exponent literal on a field, or with a backslash in any top-level key (it could decode to a field name),
// commits nothing and is listed for the host (bsh_minmax_row decides every literal and decodes every key).
//
// Commit: a wave's lanes sit in one or two sets (contiguous positions, as in the walkers), so the decided rows are folded wave-wide per
// distinct set among the lanes (a ballot loop) and one lane issues a signed 64-bit atomic min, a signed 64-bit atomic max and the
// present store per (set, field): a million rows of one block are ~16 k atomics on one address, not a million.
//
// Rows that are no valid JSON object: their set's result is unspecified, but every byte read lies in the 8-byte words that hold
// [row_off[r], row_off[r + 1]) plus one word of look-ahead (IngestArgs::rows is 8-byte aligned with >= 16 readable bytes behind the
// last row), only bytes of the row itself are interpreted, every LDS index is bounded by the lane and a field number < n_fields,
// and the only global writes are the row's own set's records and the list.
//
// The per-row scanner (minmax_scan_row) is plain C++ shared by host and device: tests/minmax_scan_check.cpp runs the very same function
// on the CPU under the sanitizers, over the shapes and every truncation of them.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#include "ingest.hip.h"
#define BSG_MM_HD __host__ __device__ __forceinline__
#else
#define BSG_MM_HD inline
#endif

namespace bsg {

constexpr uint32_t kMinMaxMaxFields = 8;    // bloomgpu.h BSG_MINMAX_MAX_FIELDS
constexpr uint32_t kMinMaxMaxName = 64;     // bloomgpu.h BSG_MINMAX_MAX_NAME
constexpr int kMinMaxThreads = 256;
constexpr uint32_t kMinMaxNameBytes = kMinMaxMaxFields * kMinMaxMaxName;

// bsg_minmax on the device: min / max start at the fold's neutral elements, present at 0 (k_minmax_init)
struct MinMaxRec {
    long long min, max;
    uint32_t present, reserved;
};
static_assert(sizeof(MinMaxRec) == 24, "bsg_minmax");

struct MinMaxFields {                         // by value in the kernel arguments: 8 names of <= 64 bytes
    uint8_t name[kMinMaxNameBytes];
    uint8_t len[kMinMaxMaxFields];
    uint32_t n;
};

// scanner state bits
enum : uint32_t { MM_STR = 1u, MM_ESC = 2u, MM_KEY = 4u, MM_EXPECT_KEY = 8u, MM_VALUE = 16u, MM_NUM = 32u, MM_UNDECIDED = 64u,
                  MM_NEG = 128u, MM_OVF = 256u, MM_POINT = 512u, MM_FRAC = 1024u, MM_EXPO = 2048u };
constexpr uint32_t kMmNumBits = MM_NEG | MM_OVF | MM_POINT | MM_FRAC | MM_EXPO;
constexpr uint32_t kMmNoField = 0xFFu;

struct MinMaxScan {
    uint32_t st;                    // MM_UNDECIDED: the row commits nothing and goes to the host
    uint32_t have;                  // bit f: the row contributes st_min[f * stride], st_max[f * stride] to field f
};

// One row: bytes [pos, end) of the buffer `chunks` holds as aligned 8-byte words (readable up to the word behind the one with the
// row's last byte).  names / lens: the fields (kMinMaxMaxName bytes each); all_fields = (1 << n_fields) - 1; the caller's staging
// slots of field f are st_min[f * stride] and st_max[f * stride].
BSG_MM_HD MinMaxScan minmax_scan_row(const uint64_t *chunks, uint64_t pos, uint64_t end, const uint8_t *names, const uint8_t *lens, uint32_t all_fields,
                                     long long *st_min, long long *st_max, uint32_t stride)
{
    uint32_t st = 0, depth = 0, cand = 0, klen = 0, field = kMmNoField, have = 0;
    uint64_t mag = 0;
    if (pos < end) {
        uint64_t ci = pos >> 3;
        uint64_t cur = chunks[ci], nxt = chunks[ci + 1];     // one word ahead: its latency hides behind the bytes of this one
        while (pos < end) {
            if ((pos >> 3) != ci) { ++ci; cur = nxt; nxt = chunks[ci + 1]; }
            const uint32_t c = (uint32_t)(cur >> ((pos & 7u) * 8u)) & 0xFFu;
            if (st & MM_NUM) {                                  // the literal of a matched key
                const uint32_t d = c - (uint32_t)'0';
                if (d <= 9u || c == '.' || c == '-' || c == '+' || (c | 0x20u) == 'e') {
                    if (!(st & MM_EXPO)) {
                        if (d <= 9u) {
                            if (st & MM_POINT) { if (d) st |= MM_FRAC; }
                            else {
                                if (mag > 1844674407370955161ULL || (mag == 1844674407370955161ULL && d > 5u)) st |= MM_OVF;   // mag * 10 + d > 2^64 - 1
                                mag = mag * 10u + d;
                            }
                        }
                        else if (c == '-') st |= MM_NEG;
                        else if (c == '.') st |= MM_POINT;
                        else st |= MM_EXPO;
                    }
                    ++pos;
                    continue;
                }
                // the literal ended: stage floor and ceil, clamped (|v| = mag + f, 0 <= f < 1, f != 0 iff MM_FRAC)
                st &= ~MM_NUM;
                if (st & MM_EXPO) st |= MM_UNDECIDED;
                else {
                    const bool ovf = st & MM_OVF, frac = st & MM_FRAC;
                    const bool below = (st & MM_NEG) && (mag != 0ull || frac || ovf);      // -0 and -0.0 are 0
                    long long mn, mx;
                    if (!below) {
                        const bool big = ovf || mag > (uint64_t)INT64_MAX;
                        mn = big ? INT64_MAX : (long long)mag;
                        mx = (big || (frac && mag == (uint64_t)INT64_MAX)) ? INT64_MAX : (long long)(mag + (frac ? 1u : 0u));
                    } else {
                        const uint64_t lim = 1ull << 63;                                    // |INT64_MIN|
                        const bool big = ovf || mag > lim;
                        mx = big ? INT64_MIN : (long long)(0ull - mag);                     // ceil(-(mag + f)) = -mag
                        mn = (big || mag + (frac ? 1u : 0u) >= lim) ? INT64_MIN : (long long)(0ull - (mag + (frac ? 1u : 0u)));
                    }
                    st_min[field * stride] = mn;                                            // field < n_fields: it came out of cand
                    st_max[field * stride] = mx;
                    have |= 1u << field;
                }
                // c itself is looked at below
            }
            if (st & MM_STR) {
                if (!(st & MM_ESC) && (!(st & MM_KEY) || cand == 0u)) {
                    // most bytes of a row lie inside strings nobody compares: the run up to the word's first quote or backslash at once
                    const uint64_t w = cur >> ((pos & 7u) * 8u);       // the bytes from pos on, lowest first (zero bytes come in at the top)
                    const uint64_t q = w ^ 0x2222222222222222ULL, b = w ^ 0x5C5C5C5C5C5C5C5CULL;
                    const uint64_t hit = ((q - 0x0101010101010101ULL) & ~q & 0x8080808080808080ULL) | ((b - 0x0101010101010101ULL) & ~b & 0x8080808080808080ULL);
                    uint64_t n = hit ? (uint64_t)(__builtin_ctzll(hit) >> 3) : 8u;    // its lowest set bit marks the first such byte exactly
                    const uint64_t in_word = 8u - (pos & 7u);
                    if (n > in_word) n = in_word;
                    if (n > end - pos) n = end - pos;
                    if (n) { pos += n; continue; }                    // (a key no field can be any more: its length no longer matters)
                }
                if (st & MM_ESC) st &= ~MM_ESC;
                else if (c == '\\') { st |= MM_ESC; if (st & MM_KEY) st |= MM_UNDECIDED; }
                else if (c == '"') {
                    if (st & MM_KEY) {                          // the field whose name is exactly these bytes, if any (names are distinct)
                        field = kMmNoField;
                        for (uint32_t m = cand; m; m &= m - 1u) {
                            const uint32_t f = (uint32_t)__builtin_ctz(m);
                            if (lens[f] == klen) field = f;
                        }
                    }
                    st &= ~(MM_STR | MM_KEY);
                } else if (st & MM_KEY) {
                    for (uint32_t m = cand; m; m &= m - 1u) {
                        const uint32_t f = (uint32_t)__builtin_ctz(m);
                        if (klen >= lens[f] || names[f * kMinMaxMaxName + klen] != c) cand &= ~(1u << f);   // klen < len <= 64
                    }
                    ++klen;
                }
                ++pos;
                continue;
            }
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r') { ++pos; continue; }
            if (st & MM_VALUE) {                                // the first byte of a top-level member's value
                st &= ~MM_VALUE;
                if (field != kMmNoField) {
                    if (c == '-' || c - (uint32_t)'0' <= 9u) {
                        st = (st & ~kMmNumBits) | MM_NUM;
                        mag = 0;
                        continue;                               // fed to the number branch above
                    }
                    have &= ~(1u << field);                     // the last member with this key is no number: it contributes nothing
                }
            }
            if (c == '"') {
                st |= MM_STR;
                if (depth == 1u && (st & MM_EXPECT_KEY)) { st = (st & ~MM_EXPECT_KEY) | MM_KEY; cand = all_fields; klen = 0; }
            }
            else if (c == '{') { if (++depth == 1u) st |= MM_EXPECT_KEY; }
            else if (c == '[') ++depth;
            else if (c == '}' || c == ']') { if (depth) --depth; }
            else if (c == ',') { if (depth == 1u) st |= MM_EXPECT_KEY; }
            else if (c == ':') { if (depth == 1u) st |= MM_VALUE; }
            ++pos;
        }
    }
    return MinMaxScan{st, have};
}

#ifdef __HIPCC__
struct MinMaxArgs {
    const uint8_t *rows;            // as IngestArgs
    const uint64_t *row_off;
    const uint32_t *set_first_row;  // RowsGrouped only
    MinMaxRec *result;              // [n_sets * n_fields]
    uint32_t *fallback_rows;        // rows the scanner does not decide (a list of its own: the walker's is rewound when a chunk is walked again)
    uint32_t *n_fallback;
    uint32_t n_sets;
    uint32_t row_first, row_end;
    uint32_t rows_per_wave;         // multiple of 64
};

// staged contributions: mins [field][thread], then maxes [field][thread] (a lane's 8-byte slots are neighbours of its neighbours')
__host__ __device__ constexpr uint32_t minmax_lds_bytes(uint32_t n_fields) { return n_fields * kMinMaxThreads * 16u + kMinMaxNameBytes + 16u; }

__global__ __launch_bounds__(256) void k_minmax_init(MinMaxRec *rec, uint32_t first, uint32_t end)
{
    const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
    if (i < end) rec[i] = MinMaxRec{INT64_MAX, INT64_MIN, 0u, 0u};
}

__device__ __forceinline__ long long wave_min_i64(long long v)
{
    for (int o = 32; o; o >>= 1) { const long long x = __shfl_xor(v, o, 64); v = x < v ? x : v; }
    return v;
}
__device__ __forceinline__ long long wave_max_i64(long long v)
{
    for (int o = 32; o; o >>= 1) { const long long x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}

template <class ROWS>
__device__ __forceinline__ void minmax_rows_body(const MinMaxArgs &a, const MinMaxFields &fl, const ROWS &rows)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t mm_lds[];
    const uint32_t nf = fl.n;
    long long *st_min = (long long *)mm_lds, *st_max = st_min + nf * kMinMaxThreads;
    uint8_t *names = (uint8_t *)(st_max + nf * kMinMaxThreads), *lens = names + kMinMaxNameBytes;
    for (uint32_t i = threadIdx.x; i < kMinMaxNameBytes; i += kMinMaxThreads) names[i] = fl.name[i];
    if (threadIdx.x < kMinMaxMaxFields) lens[threadIdx.x] = fl.len[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t all_fields = (1u << nf) - 1u;
    const uint64_t wave = (uint64_t)blockIdx.x * (kMinMaxThreads / 64) + (threadIdx.x >> 6);
    const uint64_t run_begin = a.row_first + wave * a.rows_per_wave;
    const uint32_t run_end = (uint32_t)(run_begin + a.rows_per_wave < a.row_end ? run_begin + a.rows_per_wave : a.row_end);
    const uint64_t *chunks = reinterpret_cast<const uint64_t *>(a.rows);
    for (uint64_t tile = run_begin; tile < run_end; tile += 64) {
        uint32_t r = (uint32_t)tile + lane;
        const bool live = r < run_end;
        uint32_t set = 0;
        if constexpr (ROWS::kBySet) {
            set = live ? rows.set_of_order[r] : 0u;
            r = live ? rows.row_order[r] : 0u;
        } else {
            uint32_t hi = a.n_sets;             // last s with set_first_row[s] <= r, as the walkers
            while (live && hi - set > 1) {
                const uint32_t mid = (set + hi) >> 1;
                if (a.set_first_row[mid] <= r) set = mid; else hi = mid;
            }
        }
        uint64_t pos = live ? a.row_off[r] : 0;
        const uint64_t end = live ? a.row_off[r + 1] : 0;
        const MinMaxScan sc = minmax_scan_row(chunks, pos, end, names, lens, all_fields, st_min + threadIdx.x, st_max + threadIdx.x, (uint32_t)kMinMaxThreads);
        const uint32_t st = sc.st, have = sc.have;
        // commit: nothing of an undecided row; the decided rows folded per distinct set among the lanes
        if (live && (st & MM_UNDECIDED)) {
            const uint32_t slot = __hip_atomic_fetch_add(a.n_fallback, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.fallback_rows[slot] = r;
        }
        const uint32_t hv = (live && !(st & MM_UNDECIDED)) ? have : 0u;
        uint64_t pending = __ballot(hv != 0u);
        while (pending) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(pending);
            const uint32_t s = (uint32_t)__shfl((int)set, (int)leader, 64);
            const bool in = hv != 0u && set == s;
            for (uint32_t f = 0; f < nf; ++f) {
                const bool has = in && ((hv >> f) & 1u);
                if (__ballot(has) == 0ull) continue;
                const long long mn = wave_min_i64(has ? st_min[f * kMinMaxThreads + threadIdx.x] : INT64_MAX);
                const long long mx = wave_max_i64(has ? st_max[f * kMinMaxThreads + threadIdx.x] : INT64_MIN);
                if (lane == leader) {
                    MinMaxRec *rec = a.result + (size_t)s * nf + f;
                    __hip_atomic_fetch_min(&rec->min, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_max(&rec->max, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    rec->present = 1u;
                }
            }
            pending &= ~__ballot(in);
        }
    }
}

__global__ __launch_bounds__(kMinMaxThreads) void k_minmax_rows(const MinMaxArgs a, const MinMaxFields fl) { minmax_rows_body(a, fl, RowsGrouped{}); }
__global__ __launch_bounds__(kMinMaxThreads) void k_minmax_rows_sets(const MinMaxArgs a, const MinMaxFields fl, const RowsBySet rows)
{
    minmax_rows_body(a, fl, rows);
}

#endif  // __HIPCC__

}  // namespace bsg
