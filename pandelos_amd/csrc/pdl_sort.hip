// pdl_sort.hip — K-sort: stable LSD radix sort of (key, u32 value) pairs, hand-written for gfx950.
//
// Counterpart of counting_sort_ext (ig/native/library.cpp:172-187): one stable counting pass per 8-bit
// digit.  The reference copies the whole 16-byte record vector per pass and runs single-threaded; here a
// pass is three launches over 4096-element tiles:
//
//   k_rs_hist     per-tile digit histogram in LDS (wave-coalesced key reads)      -> counts[digit][tile]
//   (scan)        exclusive scan of counts in digit-major order (pdl_scan.h)      -> offs[digit][tile]
//   k_rs_scatter  stable in-tile ranking without atomics on the data path:
//                   a tile is 4 waves x 16 rounds x 64 lanes, ordered wave-major, so every global read is a
//                   coalesced 64-element run; in a round the lanes holding the same digit find each other
//                   with 8 wave ballots (one per digit bit), rank = popcount of equal lanes below + the
//                   wave's running count of that digit (private LDS counters, no contention);
//                 elements are then placed digit-sorted in LDS and written out as coalesced runs to
//                   offs[digit][tile] + position inside the tile's digit run.
//
// HBM traffic per pass and element: key read twice (histogram, scatter), value read once, both written
// once: 3 * sizeof(key) + 8 bytes.  Stability makes the composition of passes an LSD sort and keeps the
// gene order of equal ranks (the k-mer stream is produced in gene order), which is what replaces the
// reference's seq-byte passes (library.cpp:270-274).
#include "pdl_sort.h"
#include "pdl_scan.h"

constexpr int RS_THREADS = 256;
constexpr int RS_ROUNDS = 16;
constexpr int RS_TILE = RS_THREADS * RS_ROUNDS;           // 4096 elements
constexpr int RS_WAVE_SPAN = PDL_WAVE * RS_ROUNDS;        // elements of one wave inside a tile
constexpr int RS_BINS = 256;
static_assert(RS_THREADS == RS_BINS, "one thread per digit in the tile-level scans");

template <class KeyT>
__global__ __launch_bounds__(RS_THREADS) void k_rs_hist(const KeyT *__restrict__ keys, uint64_t n_bound, const uint64_t *d_n, uint32_t shift,
                                                        uint32_t n_tiles, uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_h[RS_BINS];
    const uint64_t n = scan_count(n_bound, d_n);         // the count may live on the device (grid sized for the bound)
    const uint64_t base = (uint64_t) blockIdx.x * RS_TILE;
    if (base >= n) {                                     // (uniform) tile past the end
        counts[(size_t) threadIdx.x * n_tiles + blockIdx.x] = 0;
        return;
    }
    s_h[threadIdx.x] = 0;
    pdl_sync();
    KeyT key[RS_ROUNDS];
#pragma unroll
    for (int j = 0; j < RS_ROUNDS; j++) {            // all sixteen loads in flight before the first LDS atomic
        const uint64_t i = base + (uint64_t) j * RS_THREADS + threadIdx.x;
        key[j] = keys[i < n ? i : n - 1];
    }
#pragma unroll
    for (int j = 0; j < RS_ROUNDS; j++) {
        const uint64_t i = base + (uint64_t) j * RS_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&s_h[radix_digit(key[j], shift)], 1u);
    }
    pdl_sync();
    counts[(size_t) threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

struct RsCountFlag {
    const uint32_t *counts;
    __device__ uint32_t operator()(uint64_t i) const { return counts[i]; }
};
struct RsOffsApply {
    uint32_t *offs;
    __device__ void operator()(uint64_t i, uint32_t, uint32_t prefix) const { offs[i] = prefix; }
};

// The offsets of a pass in ONE launch: workgroup d takes the row counts[d][0 .. n_tiles) — the whole bound, tiles past a
// device-side count hold zeros — and leaves the row's exclusive prefix in offs[d][..] and its sum in digit_total[d].  The
// scatter turns the 256 sums into the digit bases itself (radix_tile_scan).  A thread holds RO_ITEMS consecutive entries
// in registers, so a row of n_tiles entries takes n_tiles / RO_TRIP trips of one block scan each.
constexpr int RO_THREADS = 1024, RO_ITEMS = 4, RO_TRIP = RO_THREADS * RO_ITEMS;
constexpr uint32_t RO_MAX_TILES = 65536;                 // longer rows (16 trips): the three-launch scan over the whole table
__global__ __launch_bounds__(RO_THREADS) void k_rs_offsets(const uint32_t *__restrict__ counts, uint32_t *__restrict__ offs, uint32_t n_tiles,
                                                           uint32_t *__restrict__ digit_total) {
    __shared__ uint32_t s_wave[17];
    const uint32_t *row = counts + (size_t) blockIdx.x * n_tiles;
    uint32_t *out = offs + (size_t) blockIdx.x * n_tiles;
    uint32_t carry = 0;                                  // (uniform) sum of the trips before
    for (uint32_t base = 0; base < n_tiles; base += RO_TRIP) {
        const uint32_t i0 = base + threadIdx.x * RO_ITEMS;
        uint32_t v[RO_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < RO_ITEMS; j++) { v[j] = i0 + j < n_tiles ? row[i0 + j] : 0u; sum += v[j]; }
        uint32_t total;
        uint32_t ex = block_exclusive_scan_u32(sum, s_wave, total) + carry;
#pragma unroll
        for (int j = 0; j < RO_ITEMS; j++) { if (i0 + j < n_tiles) out[i0 + j] = ex; ex += v[j]; }
        carry += total;
    }
    if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
}

// NBITS: significant bits of this pass's digit (the last pass of a sort may have fewer than 8), see radix_rank_rounds.
template <class KeyT, class ValT, int NBITS>
__global__ __launch_bounds__(RS_THREADS) void k_rs_scatter(const KeyT *__restrict__ keys_in, const ValT *vals_in,
                                                           KeyT *__restrict__ keys_out, ValT *__restrict__ vals_out, uint64_t n_bound,
                                                           const uint64_t *d_n, uint32_t shift, uint32_t n_tiles, const uint32_t *__restrict__ offs,
                                                           const uint32_t *__restrict__ digit_total, uint64_t *d_total) {     // offsets from k_rs_offsets: see radix_tile_scan
    const uint64_t n = scan_count(n_bound, d_n);
    if ((uint64_t) blockIdx.x * RS_TILE >= n) {                              // (uniform) tile past the end
        if (digit_total && blockIdx.x == 0 && threadIdx.x == 0) *d_total = 0;      // (a count of zero on the device: the total is zero)
        return;
    }
    __shared__ RadixTileLds<KeyT, ValT, uint32_t> s;

    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
    const uint64_t tile_base = (uint64_t) blockIdx.x * RS_TILE;
    const uint64_t wave_base = tile_base + (uint64_t) wave * RS_WAVE_SPAN;
    s.clear_counts();
    const uint32_t goff = offs[(size_t) tid * n_tiles + blockIdx.x];
    const uint32_t dtot = digit_total ? digit_total[tid] : 0u;
    pdl_sync();

    KeyT key[RS_ROUNDS];
    ValT val[RS_ROUNDS];
    uint16_t rank[RS_ROUNDS];          // position among the wave's elements of the same digit
    // every load of the tile first, branch-free (clamped index): thirty-two loads in flight per lane.  Behind a branch or
    // an LDS store the compiler keeps program order and would wait for each round's load before ranking it.
#pragma unroll
    for (int j = 0; j < RS_ROUNDS; j++) {
        const uint64_t i = wave_base + (uint64_t) j * PDL_WAVE + lane;
        key[j] = keys_in[i < n ? i : n - 1];
    }
    if (vals_in) {                                   // uniform
#pragma unroll
        for (int j = 0; j < RS_ROUNDS; j++) {
            const uint64_t i = wave_base + (uint64_t) j * PDL_WAVE + lane;
            val[j] = vals_in[i < n ? i : n - 1];
        }
    } else {                                         // the values are the positions 0, 1, 2, ...
#pragma unroll
        for (int j = 0; j < RS_ROUNDS; j++) val[j] = (ValT) (wave_base + (uint64_t) j * PDL_WAVE + lane);
    }
    const uint64_t left = n - wave_base;             // (wave_base < n or not: an element is there when its place in the wave's span lies below)
    const uint32_t lane_left = wave_base < n ? (uint32_t) (left < RS_WAVE_SPAN ? left : RS_WAVE_SPAN) : 0u;
    const auto valid = [&](int j) { return (uint32_t) j * PDL_WAVE + lane < lane_left; };
    radix_rank_rounds<NBITS>(s.cnt[wave], key, shift, valid, rank);
    pdl_sync();
    uint32_t grand_total;
    const uint32_t tile_total = radix_tile_layout(s, goff, dtot, grand_total);       // (offsets from the three-launch scan: no digit totals, base 0)
    if (digit_total && blockIdx.x == 0 && tid == 0) *d_total = grand_total;
    pdl_sync();
    radix_tile_place(s, wave, key, val, shift, valid, rank);
    pdl_sync();
    radix_tile_write(s, shift, tile_total, keys_out, vals_out);
}

template <class KeyT, class ValT>
void pdl_sort_pairs(pdl_ctx *c, KeyT *&keys_in, KeyT *&keys_out, ValT *&vals_in, ValT *&vals_out,
                    uint64_t n, uint32_t end_bit, bool iota_values, const uint64_t *d_n, uint32_t begin_bit, bool keys_below_end_bit,
                    bool first_counts_filed) {
    if (n == 0) return;
    if (end_bit == 0) end_bit = 1;
    if (end_bit > sizeof(KeyT) * 8) end_bit = sizeof(KeyT) * 8;
    if (n >= 0xfffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "sort of %llu pairs needs 64-bit positions", (unsigned long long) n);
    const uint32_t n_tiles = (uint32_t) ((n + RS_TILE - 1) / RS_TILE);
    const size_t table = (size_t) RS_BINS * n_tiles;
    c->sort_tmp.alloc(pdl_radix_tmp_bytes(n));
    uint32_t *counts = c->sort_tmp.as<uint32_t>(), *offs = counts + table, *digit_total = offs + table;
    uint64_t *d_total = c->scalars.as<uint64_t>() + PDL_CTL_SCAN_TOTAL;
    const uint32_t passes = (end_bit + 7) / 8;
    for (uint32_t p = begin_bit / 8; p < passes; p++) {
        const uint32_t shift = p * 8;
        if (!(first_counts_filed && p == begin_bit / 8))
            hipLaunchKernelGGL((k_rs_hist<KeyT>), dim3(n_tiles), dim3(RS_THREADS), 0, c->stream, keys_in, n, d_n, shift, n_tiles, counts);
        const uint32_t *totals = pdl_radix_offsets(c, counts, offs, n_tiles, d_total, digit_total);
        const ValT *vals = (p == begin_bit / 8 && iota_values) ? (const ValT *) nullptr : vals_in;
        const auto scatter = [&](auto nbits) {
            hipLaunchKernelGGL((k_rs_scatter<KeyT, ValT, decltype(nbits)::value>), dim3(n_tiles), dim3(RS_THREADS), 0, c->stream, keys_in, vals, keys_out, vals_out,
                               n, d_n, shift, n_tiles, offs, totals, d_total);
        };
        switch (keys_below_end_bit ? std::min<uint32_t>(8, end_bit - shift) : 8u) {       // the bits the pass has to match: a compile-time count
            case 1: scatter(std::integral_constant<int, 1>()); break;
            case 2: scatter(std::integral_constant<int, 2>()); break;
            case 3: scatter(std::integral_constant<int, 3>()); break;
            case 4: scatter(std::integral_constant<int, 4>()); break;
            case 5: scatter(std::integral_constant<int, 5>()); break;
            case 6: scatter(std::integral_constant<int, 6>()); break;
            case 7: scatter(std::integral_constant<int, 7>()); break;
            default: scatter(std::integral_constant<int, 8>()); break;
        }
        PDL_HIP(hipGetLastError());
        std::swap(keys_in, keys_out);
        std::swap(vals_in, vals_out);
    }
    // the sorted pairs are in the buffers the last pass wrote = (keys_in, vals_in) after the swap; hand them
    // back as the "out" pair
    std::swap(keys_in, keys_out);
    std::swap(vals_in, vals_out);
}

bool pdl_radix_lean(const pdl_ctx *c, uint64_t n) {
    return c->opt_lean_radix && !c->opt_onepass_scan && (n + RS_TILE - 1) / RS_TILE <= RO_MAX_TILES;
}

const uint32_t *pdl_radix_offsets(pdl_ctx *c, const uint32_t *counts, uint32_t *offs, uint32_t n_tiles, uint64_t *d_total, uint32_t *digit_total) {
    static_assert(PDL_RADIX_TILE == RS_TILE && PDL_RADIX_BINS == RS_BINS, "the caller's kernels use the tile shape of the sort");
    if (!pdl_radix_lean(c, (uint64_t) n_tiles * RS_TILE)) {
        scan_and_apply(c, (size_t) RS_BINS * n_tiles, RsCountFlag{counts}, RsOffsApply{offs}, d_total);
        return nullptr;
    }
    hipLaunchKernelGGL(k_rs_offsets, dim3(RS_BINS), dim3(RO_THREADS), 0, c->stream, counts, offs, n_tiles, digit_total);
    PDL_HIP(hipGetLastError());
    return digit_total;
}

template void pdl_sort_pairs<uint32_t, uint32_t>(pdl_ctx *, uint32_t *&, uint32_t *&, uint32_t *&, uint32_t *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
template void pdl_sort_pairs<uint64_t, uint32_t>(pdl_ctx *, uint64_t *&, uint64_t *&, uint32_t *&, uint32_t *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
template void pdl_sort_pairs<uint32_t, unsigned long long>(pdl_ctx *, uint32_t *&, uint32_t *&, unsigned long long *&, unsigned long long *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
