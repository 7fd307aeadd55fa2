// pdl_sort.h — stable LSD radix sort of (key, value) pairs on a bit range of the key.
//
// Counterpart of counting_sort_ext (ig/native/library.cpp:172-187) and its call sites (:270-278):
// the reference sorts 16-byte records by the bytes of seq then the bytes of rank; here the k-mer
// stream is produced in gene order, so ONE stable sort on the rank bits alone yields the same
// (rank, gene) order, and a second stable sort of the deduplicated records on the gene bits yields
// the per-gene lists.
#pragma once

#include "pdl_common.h"
#include "pdl_scan.h"

// Sorts n pairs by key bits [begin_bit, end_bit) (begin_bit a multiple of 8: the passes below it were made by
// the caller, see pdl_radix_offsets).  Input in (*keys_in, *vals_in); on return the sorted
// pairs are in (*keys_out, *vals_out) — the function may swap the roles of the buffers, the
// pointers passed by reference are updated accordingly (no pass to make: the input pair is handed back as the output).
template <class KeyT, class ValT = uint32_t>       // ValT: uint32_t, or unsigned long long (an 8-byte payload carried along)
void pdl_sort_pairs(pdl_ctx *c, KeyT *&keys_in, KeyT *&keys_out, ValT *&vals_in, ValT *&vals_out,
                    uint64_t n, uint32_t end_bit, bool iota_values = false,   // iota_values: the values are 0, 1, 2, ... (vals_in is not read)
                    const uint64_t *d_n = nullptr,                            // d_n: the count lives on the device (*d_n <= n, grids sized for n)
                    uint32_t begin_bit = 0,
                    bool keys_below_end_bit = false,                          // every key < 2^end_bit (or: nothing but zeros between end_bit and the end of the last digit): a pass
                                                                              // then matches the significant bits of its digit only; else all eight (ranks that wrapped, see RankParams)
                    bool first_counts_filed = false);                         // the kernel that made the keys has filed the first pass's counts[digit * n_tiles + tile] at the head of
                                                                              // c->sort_tmp (sized by pdl_radix_tmp_bytes(n) before it ran): that pass makes no histogram of its own

// A radix pass whose elements are made by the caller's own kernel (K-ranges: the range tuples are scattered by the low gene
// byte by the kernel that builds them): tiles of PDL_RADIX_TILE source elements, counts[digit * n_tiles + tile] filled by the
// caller -> offs[digit * n_tiles + tile] = where the tile's run of that digit starts; *d_total = number of elements.
// Option "lean_radix" (the default; rows of at most 65 536 tiles, "onepass_scan" off): one launch scans every digit's row on its
// own and leaves the rows' sums in digit_total[256]; the function returns digit_total and the scatter kernel finishes the job —
// radix_tile_scan() gives each of its 256 threads the base of its digit, and workgroup 0 writes *d_total.  Otherwise: the
// three-launch scan over the whole table, offs and *d_total are final, the function returns nullptr (the scatter adds nothing).
constexpr uint32_t PDL_RADIX_TILE = 4096, PDL_RADIX_BINS = 256;
const uint32_t *pdl_radix_offsets(pdl_ctx *c, const uint32_t *counts, uint32_t *offs, uint32_t n_tiles, uint64_t *d_total, uint32_t *digit_total);
bool pdl_radix_lean(const pdl_ctx *c, uint64_t n);                 // a sort of n elements takes the one-launch offsets
// bytes of c->sort_tmp a sort of n elements works in: counts | offs | digit_total
inline size_t pdl_radix_tmp_bytes(uint64_t n) {
    return (2 * (size_t) PDL_RADIX_BINS * ((n + PDL_RADIX_TILE - 1) / PDL_RADIX_TILE) + PDL_RADIX_BINS) * sizeof(uint32_t);
}

// ---- the radix tile body -----------------------------------------------------------------------------------------------------
// One tile of a scatter pass, shared by k_rs_scatter<KeyT, ValT> (pdl_sort.hip) and k_range_scatter (pdl_groups.h): a workgroup
// of RT_THREADS = 256 threads takes RT_TILE = 4096 elements, a wave RT_ROUNDS = 16 rounds of 64 consecutive ones.  The kernel
// loads (or makes) key[j], val[j] of its lane's sixteen elements and says which of them are there (ValidF: bool operator()(int j));
// the digit of an element is (key >> shift) & 0xff.  Four parts, in this order, a barrier between each two:
//   radix_rank_rounds   rank[j] = elements of the same digit before this one in its wave; leaves the wave's digit counts
//   radix_tile_layout   the tile scan (radix_tile_scan): the waves' counts become their bases inside the digit-sorted tile,
//                       delta[d] = (where the tile's run of digit d starts in the output) - (where it starts in the tile)
//   radix_tile_place    key and value to their place in the digit-sorted tile in LDS
//   radix_tile_write    the digit-sorted tile out as coalesced runs: element e goes to delta[its digit] + e
// CntT: the waves' counters, uint32_t or uint16_t (a count is at most 1024, a base at most 4096).  Positions are 32-bit: a pass
// has fewer than 2^32 elements (pdl_sort_pairs refuses more, k_range_scatter counts records in 32 bits).
constexpr int RT_THREADS = PDL_RADIX_BINS, RT_WAVES = RT_THREADS / PDL_WAVE, RT_TILE = PDL_RADIX_TILE, RT_ROUNDS = RT_TILE / RT_THREADS, RT_BINS = PDL_RADIX_BINS;
static_assert(RT_ROUNDS == 16 && RT_WAVES == 4, "tile shape of the radix passes");

template <class KeyT, class ValT, class CntT>
struct RadixTileLds {
    unsigned long long wsum[17];            // radix_tile_scan
    ValT val[RT_TILE];
    KeyT key[RT_TILE];
    uint32_t delta[RT_BINS];
    CntT cnt[RT_WAVES][RT_BINS];

    __device__ __forceinline__ void clear_counts() {
        for (int w = 0; w < RT_WAVES; w++) cnt[w][threadIdx.x] = 0;
    }
};

template <class KeyT>
__device__ __forceinline__ uint32_t radix_digit(KeyT k, uint32_t shift) { return (uint32_t) (k >> shift) & (RT_BINS - 1); }

// NBITS: the bits of the digit that tell elements apart (8; fewer where every key of the pass has zeros above them).  The
// lanes of a round that hold another digit are collected bit by bit: y = bit b of the own digit spread over a word, m = the
// lanes whose bit b is set, so m ^ y has a 1 for every lane whose bit differs (one sign-extending bit-field extract, one
// compare, two exclusive-ors per bit, the ors folded in pairs; no branch).  The first lane of a digit files the wave's new count.
template <int NBITS, class KeyT, class CntT, class ValidF>
__device__ __forceinline__ void radix_rank_rounds(CntT *cnt /* the wave's row */, const KeyT (&key)[RT_ROUNDS], uint32_t shift, ValidF valid,
                                                  uint16_t (&rank)[RT_ROUNDS]) {
    static_assert(NBITS >= 1 && NBITS <= 8, "a digit has eight bits");
#pragma unroll
    for (int j = 0; j < RT_ROUNDS; j++) {
        const uint32_t d = radix_digit(key[j], shift);
        const uint32_t seen = cnt[d];                                // earlier rounds (own wave only: no race); read here, used behind the ballots
        const bool v = valid(j);
        const unsigned long long vm = __ballot(v);
        uint32_t diff_lo = 0, diff_hi = 0;
#pragma unroll
        for (int b = 0; b < NBITS; b++) {
            uint32_t y = (uint32_t) ((int32_t) (d << (31 - b)) >> 31);
            asm("" : "+v"(y));                                       // (the compare reads y: else the compiler tests a shifted copy of d, one instruction more)
            const unsigned long long m = __ballot(y != 0u);
            diff_lo |= (uint32_t) m ^ y;
            diff_hi |= (uint32_t) (m >> 32) ^ y;
        }
        const uint32_t same_lo = (uint32_t) vm & ~diff_lo, same_hi = (uint32_t) (vm >> 32) & ~diff_hi;      // valid lanes of the wave holding digit d in this round
        const uint32_t below_me = __builtin_amdgcn_mbcnt_hi(same_hi, __builtin_amdgcn_mbcnt_lo(same_lo, 0u));
        rank[j] = (uint16_t) (seen + below_me);
        const uint32_t now = seen + (uint32_t) __popc(same_lo) + (uint32_t) __popc(same_hi);
        if (v && below_me == 0) cnt[d] = (CntT) now;
    }
}

// After the barrier behind the ranking.  goff: offs[digit = thread][tile]; dtot: digit_total[thread] (0 where the offsets are
// final).  Returns the elements of the tile; grand_total: those of the pass (where dtot is given).
template <class KeyT, class ValT, class CntT>
__device__ __forceinline__ uint32_t radix_tile_layout(RadixTileLds<KeyT, ValT, CntT> &s, uint32_t goff, uint32_t dtot, uint32_t &grand_total) {
    const uint32_t tid = threadIdx.x;
    uint32_t tot = 0;
    uint32_t wcnt[RT_WAVES];
#pragma unroll
    for (int w = 0; w < RT_WAVES; w++) { wcnt[w] = s.cnt[w][tid]; tot += wcnt[w]; }
    uint32_t tile_total, digit_base;
    const uint32_t ex = radix_tile_scan(tot, dtot, s.wsum, tile_total, digit_base, grand_total);
    s.delta[tid] = goff + digit_base - ex;               // (mod 2^32; delta + position in the tile is the place in the output)
    uint32_t run = ex;                                   // digit runs in digit order, inside a run wave 0's elements first
#pragma unroll
    for (int w = 0; w < RT_WAVES; w++) { s.cnt[w][tid] = (CntT) run; run += wcnt[w]; }
    return tile_total;
}

template <class KeyT, class ValT, class CntT, class ValidF>
__device__ __forceinline__ void radix_tile_place(RadixTileLds<KeyT, ValT, CntT> &s, uint32_t wave, const KeyT (&key)[RT_ROUNDS], const ValT (&val)[RT_ROUNDS],
                                                 uint32_t shift, ValidF valid, const uint16_t (&rank)[RT_ROUNDS]) {
#pragma unroll
    for (int j = 0; j < RT_ROUNDS; j++) {
        if (valid(j)) {
            const uint32_t at = s.cnt[wave][radix_digit(key[j], shift)] + rank[j];
            s.key[at] = key[j];
            s.val[at] = val[j];
        }
    }
}

// After the barrier behind the placement.
template <class KeyT, class ValT, class CntT>
__device__ __forceinline__ void radix_tile_write(const RadixTileLds<KeyT, ValT, CntT> &s, uint32_t shift, uint32_t tile_total, KeyT *__restrict__ keys_out,
                                                 ValT *__restrict__ vals_out) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < RT_ROUNDS; j++) {
        const uint32_t e = j * RT_THREADS + tid;                     // coalesced over the digit-sorted tile
        if (e < tile_total) {
            const KeyT k = s.key[e];
            const uint32_t dst = s.delta[radix_digit(k, shift)] + e;
            keys_out[dst] = k;
            vals_out[dst] = s.val[e];
        }
    }
}

extern template void pdl_sort_pairs<uint32_t, uint32_t>(pdl_ctx *, uint32_t *&, uint32_t *&, uint32_t *&, uint32_t *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
extern template void pdl_sort_pairs<uint64_t, uint32_t>(pdl_ctx *, uint64_t *&, uint64_t *&, uint32_t *&, uint32_t *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
extern template void pdl_sort_pairs<uint32_t, unsigned long long>(pdl_ctx *, uint32_t *&, uint32_t *&, unsigned long long *&, unsigned long long *&, uint64_t, uint32_t, bool, const uint64_t *, uint32_t, bool, bool);
