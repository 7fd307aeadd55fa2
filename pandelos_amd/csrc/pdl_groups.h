// pdl_groups.h — K-groups + K-ranges (library.cpp:289-335): the passes over the deduplicated postings that make the per-gene
// range lists, the counters and the costs.  Included from pdl_dict.hip, whose stages launch them.
//
// The dictionary arrives as postings {gene, count} in (rank, gene) order with "opens a rank-group" in bit 31 of the count
// (set by K-rle; also the form the runs of a multi-GPU build travel in).  A group is the records from one head to the next;
// nothing is materialised about groups: every tile of GW_TILE = 1024 records (one wave) rebuilds what it needs from the bits.
//
//   k_fold_last_record  the reference's scan closes the current group at the LAST record whatever its rank (library.cpp:300-306):
//          a last record that opens a group of its own is folded into the group before it, at its gene-order place (:312-315),
//          and the head bits are put right, so that from here on the bits alone say what the reference's groups are
//   costs  k_group_costs<GENOMES, RECORD_COSTS>: no ranges; counters, and the group size of every shared record added to its
//          gene's cost (complexity-only) or its genome's lookups (the multi-GPU deal).  Extents from ballots of the head bits;
//          the groups that cross the tile's borders: a look at the records around the tile (find_head_back / find_head_fwd)
//   count  per-thread code: ranges per tile, first / last head of every tile, counters.  k_range_count<MODE>, or
//          k_range_count_hist: + a workgroup's ranges counted by the low byte of their gene (the gene sort's first histogram)
//   (scan of the counts: k_tile_prefix + k_scan_tile_scan, or the radix offsets)
//   write  extents as in the costs kernel; the groups that cross the borders are found in the per-tile heads the count pass
//          left (gt_tile_borders: two coalesced reads issued with the tile's own loads).  The postings are only read: the head
//          bits stay in them (the next genome batch counts and writes from them again; the joins mask bit 31 of a count).
//          k_group_write<MODE> files {gene, range} in record order; k_range_scatter (single-GPU build: upper
//          ranges, packed) ranks them by the low byte of the gene and files them as the gene sort's first pass would
//   k_gene_costs_lazy   reads the copy of the head bits a write pass filed, one bit per record (GroupTileArgs::head_bits)
//
// MODE 0: whole groups for the genes of a shard | 1: the postings above the record, every gene | 2: those, for the genes of
// a shard.  The gt_* bodies are shared by the kernels named in their comments: arrays by reference, no LDS of their own.
#pragma once
#include "pdl_common.h"
#include "pdl_scan.h"
#include "pdl_sort.h"

constexpr uint32_t HEAD_BIT = 0x80000000u;
constexpr uint32_t GT_NONE = 0xffffffffu;
constexpr uint32_t COST_LDS_GENOMES = 4096;
constexpr int GW_ROUNDS = 16, GW_TILE = GW_ROUNDS * PDL_WAVE, GW_THREADS = 256, GW_WAVES = GW_THREADS / PDL_WAVE;
constexpr uint32_t GW_MAX_IV = 2048;                     // gene-id intervals of a shard held in LDS (16 KiB); more: the byte table

// last head at or before pos (record 0 always is one); one wave, 64 records per step
__device__ __forceinline__ uint32_t find_head_back(const uint2 *post, uint32_t pos, uint32_t lane) {
    for (;;) {
        const uint32_t base = pos + 1 >= PDL_WAVE ? pos + 1 - PDL_WAVE : 0;
        const uint32_t idx = base + lane;
        const bool f = idx <= pos && ((post[idx <= pos ? idx : pos].y >> 31) || idx == 0);
        const unsigned long long m = __ballot(f);
        if (m) return base + 63u - (uint32_t) __clzll((long long) m);
        pos = base - 1;                                   // (base > 0 here: index 0 always answers)
    }
}
// first head at or after pos, n when there is none
__device__ __forceinline__ uint32_t find_head_fwd(const uint2 *post, uint32_t pos, uint32_t n, uint32_t lane) {
    for (uint32_t base = pos; base < n; base += PDL_WAVE) {
        const uint32_t idx = base + lane;
        const bool f = idx < n && (post[idx < n ? idx : n - 1].y >> 31);
        const unsigned long long m = __ballot(f);
        if (m) return base + (uint32_t) __ffsll((long long) m) - 1u;
    }
    return n;
}

// One workgroup.  recpos (position of each record's first occurrence in the sorted stream, for pdl_get_dictionary) moves
// along when present.
__global__ __launch_bounds__(1024) void k_fold_last_record(uint2 *__restrict__ post, uint32_t *__restrict__ recpos, const uint64_t *d_u) {
    __shared__ uint32_t s_gs, s_p;
    const uint32_t u_count = (uint32_t) *d_u;
    if (u_count < 2) return;
    const uint32_t lastp = u_count - 1;
    uint2 last = post[lastp];
    if (!(last.y >> 31)) return;                         // (uniform) the last record belongs to its group anyway, in gene order
    last.y &= ~HEAD_BIT;                                 // it never opens a group (library.cpp:300-306)
    const uint32_t last_rp = recpos ? recpos[lastp] : 0u;
    if (threadIdx.x < PDL_WAVE) {
        const uint32_t gs = find_head_back(post, lastp - 1, threadIdx.x);       // the group it joins
        if (threadIdx.x == 0) {
            uint32_t lo = gs, hi = lastp;                // first index in [gs, lastp) whose gene is above the last record's
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (post[mid].x <= last.x) lo = mid + 1; else hi = mid;
            }
            s_gs = gs; s_p = lo;
        }
    }
    pdl_sync();
    const uint32_t p = s_p, gs = s_gs;
    if (p == lastp) { if (threadIdx.x == 0) post[lastp] = last; return; }       // already in place (uniform)
    for (uint32_t hi = lastp; hi > p; hi = hi > 1024 ? hi - 1024 : 0) {
        const bool live = hi >= 1 + threadIdx.x && hi - 1 - threadIdx.x >= p;
        const uint32_t i = hi - 1 - threadIdx.x;
        uint2 v = make_uint2(0, 0);
        uint32_t rp = 0;
        if (live) { v = post[i]; if (recpos) rp = recpos[i]; }
        pdl_sync();
        if (live) { post[i + 1] = v; if (recpos) recpos[i + 1] = rp; }
        pdl_sync();
        if (hi <= 1024) break;
    }
    if (threadIdx.x == 0) {
        if (p == gs) { last.y |= HEAD_BIT; post[gs + 1].y &= ~HEAD_BIT; }       // the moved record is the group's smallest gene: it is the head now
        post[p] = last;
        if (recpos) recpos[p] = last_rp;
    }
}

struct GroupTileArgs {
    uint2 *post;
    uint64_t n_bound; const uint64_t *d_n;      // record count: on the device (at most n_bound) or n_bound itself
    const uint8_t *in_shard;                    // MODE 0, 2: the genes that get range lists, one byte per gene ...
    const uint2 *own_iv; uint32_t n_own_iv;     // ... or (n_own_iv > 0) as sorted, disjoint gene-id intervals [x, y): searched in LDS,
                                                //     where a per-record byte gather would cost 64 addresses per instruction
    uint32_t *tile_sums;                        // [tiles] count: ranges of the tile; k_tile_prefix: of the tiles before it in its block of 64
    uint32_t *chunk_sums;                       // [blocks of 64 tiles] ranges of a block; exclusive-scanned between the passes
    uint32_t n_blocks;
    uint32_t *th_first, *th_last;               // [tiles] first / last head of a tile (GT_NONE: none), count -> write
    uint32_t *key2; uint4 *tuples;              // write: sort key (gene) and the 16-byte range tuple, or ...
    unsigned long long *pay8;                   // ... (non-null) the packed 8-byte range (gt_pack_range), carried through the gene sort
                                                //     as its payload: no gather afterwards
    unsigned long long *head_bits;              // write: [tiles * 16] the head bits of the postings, one per record, filed for the lazy cost pass
    uint32_t pos_base;                          // write, packed ranges: added to every first posting (a run of a multi-GPU build: its place in the gathered dictionary)
    unsigned long long *cost;                   // per-gene total_visited (library.cpp:327): last members (write), all shared records (costs, RECORD_COSTS)
    unsigned long long *counters;               // costs, count: [0] += records in groups >= 2, [1] += such groups, [3] += records whose k-mer repeats inside its gene (count);
                                                // write: [2] += lookups of the records that belong to this context (library.cpp:327 summed: "Total cost")
    const uint32_t *genome_of; uint32_t n_genomes;
    unsigned long long *g_full, *g_upper;       // costs, GENOMES: per genome, lookups as the reference counts them / above the diagonal
};

// ---- bodies shared by the kernels ------------------------------------------------------------------------------------------

// A tile's sixteen records per lane: all loads first, branch-free.  (costs, write, k_range_scatter, the lean count; the plain count loads its own)
__device__ __forceinline__ void gt_load_tile(const uint2 *post, uint32_t t0, uint32_t n, uint32_t lane, uint2 (&po)[GW_ROUNDS]) {
#pragma unroll
    for (int j = 0; j < GW_ROUNDS; j++) {
        const uint32_t u = t0 + j * PDL_WAVE + lane;
        po[j] = post[u < n ? u : n - 1];
    }
}

// (shard modes) bit j: the gene of this lane's record of round j gets ranges — for all sixteen records at once: behind the
// ballots of a write pass each lookup would wait for the one before it.  s_iv: the shard's n_iv intervals in LDS, or
// n_iv == 0: the byte table.  (k_range_count, write)
template <int MODE>
__device__ __forceinline__ uint32_t gt_shard_mask(const GroupTileArgs &a, const uint2 *s_iv, uint32_t n_iv, const uint2 (&po)[GW_ROUNDS]) {
    if constexpr (MODE == 1) return 0xffffffffu;
    uint32_t ins = 0;
    if (n_iv) {                                          // (uniform) sixteen independent binary searches over the interval starts, in LDS
        uint32_t lo_i[GW_ROUNDS], hi_i[GW_ROUNDS];
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) { lo_i[j] = 0; hi_i[j] = n_iv; }          // last interval with start <= gene is lo_i - 1
        for (uint32_t span = n_iv; span > 0; span >>= 1) {
#pragma unroll
            for (int j = 0; j < GW_ROUNDS; j++) {
                const uint32_t mid = (lo_i[j] + hi_i[j]) >> 1;
                const bool go = lo_i[j] < hi_i[j] && s_iv[mid < n_iv ? mid : n_iv - 1].x <= po[j].x;
                if (lo_i[j] < hi_i[j]) { if (go) lo_i[j] = mid + 1; else hi_i[j] = mid; }
            }
        }
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) ins |= (uint32_t) (lo_i[j] > 0 && po[j].x < s_iv[lo_i[j] > 0 ? lo_i[j] - 1 : 0].y) << j;
    } else {
        uint8_t inb[GW_ROUNDS];
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) inb[j] = a.in_shard[po[j].x];
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) ins |= (uint32_t) (inb[j] != 0) << j;
    }
    return ins;
}

// The count of one tile, per thread: a record gets a range iff its successor does not open a group [and its gene belongs to
// the shard]; MODE 0: iff it is not alone in its group.  Leaves the tile's ranges (HIST: each also counted in s_h by the low
// byte of its gene) and its first / last head for the write pass; n_rec / n_grp / n_rep grow by the shared records, the shared
// groups and (every eighth tile, a statistic) the records whose k-mer repeats inside its gene.  (k_range_count, k_range_count_hist)
// LEAN (option "lean_records"): sixteen records of a lane are sixteen BITS.  The successor's head bit is not loaded a second
// time — the lane above holds it in the same round, lane 0 in the next round for lane 63: ONE DPP move hands over all sixteen;
// only the tile's last record loads its successor's (17 loads per lane, not 32) — and shared / range / group are mask
// arithmetic and three popcounts per tile where the plain form spends about forty vector instructions per record.
template <int MODE, bool HIST, bool LEAN>
__device__ __forceinline__ void gt_count_tile(const GroupTileArgs &a, uint32_t tile, uint32_t n, uint32_t lane, const uint2 *s_iv, uint32_t n_iv, uint32_t *s_h,
                                              uint32_t &n_rec, uint32_t &n_grp, uint32_t &n_rep) {
    const uint32_t t0 = tile * GW_TILE;
    uint2 po[GW_ROUNDS];
    uint32_t cnt = 0, first_h = GT_NONE, last_h = 0, any_h = 0;
    if constexpr (LEAN) {
        gt_load_tile(a.post, t0, n, lane, po);
        const uint32_t ub = t0 + GW_TILE;                // the successor of the tile's last record (clamped as every index)
        const uint32_t ylast = a.post[ub < n ? ub : n - 1].y;
        const uint32_t ins = gt_shard_mask<MODE>(a, s_iv, n_iv, po);
        uint32_t headm = 0;                              // bit j: this lane's record of round j opens a group
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) headm |= (po[j].y >> 31) << j;
        const uint32_t first_lane = (uint32_t) __builtin_amdgcn_readfirstlane((int) headm);
        uint32_t nextm = wave_next_u32(headm, first_lane >> 1 | (ylast >> 31) << (GW_ROUNDS - 1));      // bit j: its successor does
        uint32_t livem = (1u << GW_ROUNDS) - 1u;
        if (ub >= n) {                                   // (uniform) the last tile: records past the end, and the end as a successor
            livem = 0;
#pragma unroll
            for (int j = 0; j < GW_ROUNDS; j++) {
                const uint32_t u = t0 + j * PDL_WAVE + lane;
                livem |= (uint32_t) (u < n) << j;
                nextm |= (uint32_t) (u + 1 >= n) << j;
            }
        }
        const uint32_t head = headm & livem;
        const uint32_t shared = livem & ~(head & nextm);                      // not alone in its group
        uint32_t r = MODE == 0 ? shared : livem & ~nextm;
        if constexpr (MODE == 0 || MODE == 2) r &= ins;
        if constexpr (HIST) {
#pragma unroll
            for (int j = 0; j < GW_ROUNDS; j++) { if ((r >> j) & 1u) atomicAdd(&s_h[po[j].x & (PDL_RADIX_BINS - 1)], 1u); }
        }
        cnt = (uint32_t) __builtin_popcount(r);
        n_rec += (uint32_t) __builtin_popcount(shared); n_grp += (uint32_t) __builtin_popcount(head & ~nextm);
        if (head) {
            first_h = t0 + (uint32_t) __builtin_ctz(head) * PDL_WAVE + lane;
            last_h = t0 + (31u - (uint32_t) __builtin_clz(head)) * PDL_WAVE + lane;
            any_h = 1;
        }
    } else {
        uint32_t ynext[GW_ROUNDS];
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) {            // all loads first, branch-free
            const uint32_t u = t0 + j * PDL_WAVE + lane;
            po[j] = a.post[u < n ? u : n - 1];
            ynext[j] = a.post[u + 1 < n ? u + 1 : n - 1].y;
        }
        const uint32_t ins = gt_shard_mask<MODE>(a, s_iv, n_iv, po);
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) {
            const uint32_t u = t0 + j * PDL_WAVE + lane;
            const bool live = u < n;
            const bool head = live && (po[j].y >> 31);
            const bool next_head = u + 1 >= n || (ynext[j] >> 31);       // the successor opens a group, or is the end
            const bool shared = live && !(head && next_head);
            bool r = MODE == 0 ? shared : (live && !next_head);
            if constexpr (MODE == 0 || MODE == 2) r = r && ((ins >> j) & 1u);
            if constexpr (HIST) { if (r) atomicAdd(&s_h[po[j].x & (PDL_RADIX_BINS - 1)], 1u); }
            cnt += r;
            n_rec += shared; n_grp += head && !next_head;
            if (head) { first_h = min(first_h, u); last_h = max(last_h, u); any_h = 1; }
        }
    }
    if ((tile & 7u) == 0) {                              // (uniform)
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) n_rep += 8u * (uint32_t) (t0 + j * PDL_WAVE + lane < n && (po[j].y & ~HEAD_BIT) >= 2u);
    }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) {
        cnt += __shfl_xor(cnt, d, PDL_WAVE);
        first_h = min(first_h, (uint32_t) __shfl_xor((int) first_h, d, PDL_WAVE));
        last_h = max(last_h, (uint32_t) __shfl_xor((int) last_h, d, PDL_WAVE));
        any_h |= (uint32_t) __shfl_xor((int) any_h, d, PDL_WAVE);
    }
    if (lane == 0) { a.tile_sums[tile] = cnt; a.th_first[tile] = first_h; a.th_last[tile] = any_h ? last_h : GT_NONE; }
}

// A thread's n_rec / n_grp [/ n_rep] into counters[0] / [1] [/ [3]]: one atomic per workgroup and counter (s_red[2] zeroed
// before, a barrier in between).  (costs, k_range_count, k_range_count_hist)
template <bool REPEATS>
__device__ __forceinline__ void gt_flush_counts(const GroupTileArgs &a, uint32_t *s_red, uint32_t n_rec, uint32_t n_grp, uint32_t n_rep) {
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1);
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) {
        n_rec += __shfl_xor(n_rec, d, PDL_WAVE); n_grp += __shfl_xor(n_grp, d, PDL_WAVE);
        if constexpr (REPEATS) n_rep += __shfl_xor(n_rep, d, PDL_WAVE);
    }
    if (lane == 0) {
        atomicAdd(&s_red[0], n_rec); atomicAdd(&s_red[1], n_grp);
        if constexpr (REPEATS) { if (n_rep) atomicAdd(&a.counters[3], (unsigned long long) n_rep); }
    }
    pdl_sync();
    if (tid < 2 && s_red[tid]) atomicAdd(&a.counters[tid], (unsigned long long) s_red[tid]);
}

// bit l of m[j]: the record of lane l in round j opens a group.  (costs, write, k_range_scatter)
__device__ __forceinline__ void gt_head_masks(const uint2 (&po)[GW_ROUNDS], uint32_t t0, uint32_t n, uint32_t lane, unsigned long long (&m)[GW_ROUNDS]) {
#pragma unroll
    for (int j = 0; j < GW_ROUNDS; j++) m[j] = __ballot(t0 + j * PDL_WAVE + lane < n && (po[j].y >> 31));
}

// Write side, the groups that cross the tile's borders: the count pass's per-tile heads answer — the nearest tile before /
// after with a head, 64 tiles per look (two coalesced reads, where a look at the records around the tile is a dependent walk).
// gt_load_borders issues the first look (with the tile's own loads); gt_tile_borders gives `before` (head of the group
// that runs into the tile) and `after` (end of the group that runs out of it), wave-uniform.  (write, k_range_scatter)
__device__ __forceinline__ void gt_load_borders(const GroupTileArgs &a, uint32_t tile, uint32_t tiles, uint32_t lane, uint32_t &hb, uint32_t &ha) {
    hb = lane < tile ? a.th_last[tile - 1 - lane] : GT_NONE;                    // lane 0 = the tile just before
    ha = tile + 1 + lane < tiles ? a.th_first[tile + 1 + lane] : GT_NONE;
}
__device__ __forceinline__ void gt_tile_borders(const GroupTileArgs &a, uint32_t tile, uint32_t tiles, uint32_t t0, uint32_t n, unsigned long long m0, uint32_t lane,
                                                uint32_t hb, uint32_t ha, uint32_t &before, uint32_t &after) {
    before = t0;
    if (!(m0 & 1ull)) {                                  // (uniform) the tile starts inside a group (t0 > 0: record 0 is a head)
        unsigned long long hm = __ballot(hb != GT_NONE);
        if (hm) before = (uint32_t) __shfl((int) hb, __ffsll((long long) hm) - 1, PDL_WAVE);
        else {
            before = 0;
            for (uint32_t hi = tile >= PDL_WAVE ? tile - PDL_WAVE : 0; hi > 0;) {                    // further back, 64 tiles per step
                const uint32_t base = hi >= PDL_WAVE ? hi - PDL_WAVE : 0, idx = base + lane;
                const uint32_t v = idx < hi ? a.th_last[idx] : GT_NONE;
                hm = __ballot(v != GT_NONE);
                if (hm) { before = (uint32_t) __shfl((int) v, 63 - __clzll((long long) hm), PDL_WAVE); break; }
                hi = base;
            }
        }
    }
    unsigned long long hm = __ballot(ha != GT_NONE);
    if (hm) after = (uint32_t) __shfl((int) ha, __ffsll((long long) hm) - 1, PDL_WAVE);
    else {
        after = n;
        for (uint32_t lo = tile + 1 + PDL_WAVE; lo < tiles; lo += PDL_WAVE) {
            const uint32_t idx = lo + lane;
            const uint32_t v = idx < tiles ? a.th_first[idx] : GT_NONE;
            hm = __ballot(v != GT_NONE);
            if (hm) { after = (uint32_t) __shfl((int) v, __ffsll((long long) hm) - 1, PDL_WAVE); break; }
        }
    }
    before = (uint32_t) __builtin_amdgcn_readfirstlane((int) before);        // (uniform by construction: keep them in scalar registers)
    after = (uint32_t) __builtin_amdgcn_readfirstlane((int) after);
}

// The extent walk of a tile.  gt_next_heads: nextr[j] = first head in the rounds after round j, `after` when there is none
// (scalar scan from the back).  gt_round_extent: [gs, ge) of the group this lane's record of round j belongs to, by bit
// scans of the round's mask; pr = last head before the round (`before` to start with), moved past the round.
// (costs, write, k_range_scatter)
__device__ __forceinline__ void gt_next_heads(const unsigned long long (&m)[GW_ROUNDS], uint32_t t0, uint32_t after, uint32_t (&nextr)[GW_ROUNDS]) {
    uint32_t nx = after;
#pragma unroll
    for (int j = GW_ROUNDS - 1; j >= 0; j--) {
        nextr[j] = nx;
        if (m[j]) nx = t0 + j * PDL_WAVE + (uint32_t) __ffsll((long long) m[j]) - 1u;
    }
}
__device__ __forceinline__ void gt_round_extent(unsigned long long mj, uint32_t r0, uint32_t lane, uint32_t nextr_j, uint32_t &pr, uint32_t &gs, uint32_t &ge) {
    const unsigned long long le_mask = (2ull << lane) - 1ull;
    const unsigned long long at_or_below = mj & le_mask, above = mj & ~le_mask;
    gs = at_or_below ? r0 + 63u - (uint32_t) __clzll((long long) at_or_below) : pr;
    ge = above ? r0 + (uint32_t) __ffsll((long long) above) - 1u : nextr_j;
    if (mj) pr = r0 + 63u - (uint32_t) __clzll((long long) mj);
}

// Write side of a round: the round's head bits are filed in head_bits for the lazy cost pass; the postings are only read
// (the bit stays where K-rle put it: clearing it made the pass write back every line of the postings it had just read, and
// whoever reads a count masks it).  Returns the record's own count.  (write, k_range_scatter)
__device__ __forceinline__ uint32_t gt_take_head(const GroupTileArgs &a, uint32_t tile, int j, uint32_t y, unsigned long long mj, uint32_t lane) {
    if (a.head_bits && lane == 0) a.head_bits[(size_t) tile * GW_ROUNDS + j] = mj;
    return y & PDL_COUNT_MASK;
}

// the packed 8-byte range: first posting | (postings + (min(own count, 1023) << 22)) << 32
__device__ __forceinline__ unsigned long long gt_pack_range(uint32_t start, uint32_t len, uint32_t cnt, uint32_t pos_base) {
    return (unsigned long long) (start + pos_base) | ((unsigned long long) (len | (min(cnt, 1023u) << 22)) << 32);
}

// ---- costs ---------------------------------------------------------------------------------------------------------------------
// One WAVE per tile, no LDS and no barrier on the data path: the head bits of a round of 64 records are one ballot (a scalar
// register pair); previous / next head of a record come from bit scans of its round's mask, from scalar scans over the
// rounds, and — for the groups that cross the tile's borders — from a look at the records around the tile (the head bits
// are all there: nothing is written to the postings).  Leaves nothing for a write pass.
template <bool GENOMES, bool RECORD_COSTS>
__global__ __launch_bounds__(GW_THREADS) void k_group_costs(GroupTileArgs a) {
    __shared__ uint32_t s_red[2];
    extern __shared__ unsigned long long s_dyn[];        // GENOMES with <= COST_LDS_GENOMES genomes: full[G] | upper[G]
    unsigned long long *s_full = s_dyn, *s_upper = s_dyn + a.n_genomes;
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1);
    const uint32_t gw = blockIdx.x * GW_WAVES + tid / PDL_WAVE;                  // this wave's index = its chunk of tiles
    const uint32_t n = (uint32_t) scan_count(a.n_bound, a.d_n);
    const uint32_t tiles = (n + GW_TILE - 1) / GW_TILE;
    const bool lds_table = GENOMES && a.n_genomes <= COST_LDS_GENOMES;
    if constexpr (GENOMES) { if (lds_table) { for (uint32_t i = tid; i < 2 * a.n_genomes; i += GW_THREADS) s_dyn[i] = 0; } }
    if (tid < 2) s_red[tid] = 0;
    pdl_sync();
    uint32_t n_rec = 0, n_grp = 0;
    // Tiles are dealt round-robin over the waves: the waves in flight read neighbouring tiles (a wave that owned a run of
    // consecutive tiles kept every wave on its own far-apart addresses, and the pass at a quarter of the streaming rate).
    for (uint32_t tile = gw; tile < tiles; tile += gridDim.x * GW_WAVES) {
        const uint32_t t0 = tile * GW_TILE, t1 = min(t0 + (uint32_t) GW_TILE, n);
        uint2 po[GW_ROUNDS];
        gt_load_tile(a.post, t0, n, lane, po);
        const uint32_t pu = t1 + lane;                   // the 64 records behind the tile say where the group that runs out of it ends
        const uint32_t peek = pu < n ? a.post[pu].y >> 31 : 0u;
        unsigned long long m[GW_ROUNDS];
        gt_head_masks(po, t0, n, lane, m);
        uint32_t before = t0, after;
        if (!(m[0] & 1ull)) before = find_head_back(a.post, t0 - 1, lane);       // (uniform) the tile starts inside a group (t0 > 0: record 0 is a head)
        const unsigned long long pm = __ballot(peek != 0);
        if (pm) after = t1 + (uint32_t) __ffsll((long long) pm) - 1u;
        else if (t1 + PDL_WAVE >= n) after = n;
        else after = find_head_fwd(a.post, t1 + PDL_WAVE, n, lane);
        before = (uint32_t) __builtin_amdgcn_readfirstlane((int) before);        // (uniform by construction: keep them in scalar registers)
        after = (uint32_t) __builtin_amdgcn_readfirstlane((int) after);
        uint32_t nextr[GW_ROUNDS];
        gt_next_heads(m, t0, after, nextr);
        uint32_t pr = before;
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) {
            const uint32_t u = t0 + j * PDL_WAVE + lane;
            uint32_t gs, ge;
            gt_round_extent(m[j], t0 + j * PDL_WAVE, lane, nextr[j], pr, gs, ge);
            const bool shared = u < n && ge - gs >= 2;
            n_rec += shared; n_grp += shared && u == gs;
            if constexpr (RECORD_COSTS) { if (shared) atomicAdd(&a.cost[po[j].x], (unsigned long long) (ge - gs)); }
            if constexpr (GENOMES) {
                if (shared) {
                    const uint32_t gen = a.genome_of[po[j].x];
                    const unsigned long long full = ge - gs, up = ge - u - 1;
                    if (lds_table) { atomicAdd(&s_full[gen], full); if (up) atomicAdd(&s_upper[gen], up); }
                    else { atomicAdd(&a.g_full[gen], full); if (up) atomicAdd(&a.g_upper[gen], up); }
                }
            }
        }
    }
    gt_flush_counts<false>(a, s_red, n_rec, n_grp, 0u);
    if constexpr (GENOMES) {
        if (lds_table) for (uint32_t i = tid; i < a.n_genomes; i += GW_THREADS) {
            if (s_full[i]) atomicAdd(&a.g_full[i], s_full[i]);
            if (s_upper[i]) atomicAdd(&a.g_upper[i], s_upper[i]);
        }
    }
}

// Per-gene total_visited (library.cpp:327: every record of a group with >= 2 records adds the group size to its gene)
// made on demand from the head bits a write pass kept — only pdl_sequence_costs / pdl_genome_cost ask for it once the
// ranges travel packed.  One thread per record; the extents come from word scans of the bit array.
__global__ __launch_bounds__(256) void k_gene_costs_lazy(const uint2 *__restrict__ post, const unsigned long long *__restrict__ head_bits,
                                                         uint32_t n, unsigned long long *__restrict__ cost) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    // word layout: tile t, round j -> word t * 16 + j holds records t * 1024 + j * 64 .. +63  == record >> 6
    const uint32_t w = u >> 6, b = u & 63u, words = (n + 63) >> 6;
    uint32_t gs, ge;
    {
        unsigned long long m = head_bits[w] & ((2ull << b) - 1ull);
        uint32_t ww = w;
        while (!m && ww > 0) m = head_bits[--ww];
        gs = m ? ww * 64u + 63u - (uint32_t) __clzll((long long) m) : 0u;
    }
    {
        unsigned long long m = b == 63 ? 0ull : head_bits[w] & ~((2ull << b) - 1ull);
        uint32_t ww = w;
        while (!m && ww + 1 < words) m = head_bits[++ww];
        ge = m ? ww * 64u + (uint32_t) __ffsll((long long) m) - 1u : n;
        if (ge > n) ge = n;
    }
    if (ge - gs >= 2) atomicAdd(&cost[post[u].x], (unsigned long long) (ge - gs));
}

// ---- count ---------------------------------------------------------------------------------------------------------------------
// Per-thread code (the mask arithmetic of the costs / write kernels keeps a wave's uniform values in vector registers and
// ran at a quarter of the streaming rate).  One wave per tile, tiles dealt round-robin over the waves.
template <int MODE, bool LEAN>
__global__ __launch_bounds__(GW_THREADS) void k_range_count(GroupTileArgs a) {
    extern __shared__ unsigned long long s_dyn[];        // shard modes: the intervals
    __shared__ uint32_t s_red[2];
    uint2 *s_iv = reinterpret_cast<uint2 *>(s_dyn);
    const uint32_t n_iv = (MODE == 0 || MODE == 2) ? a.n_own_iv : 0u;
    if constexpr (MODE == 0 || MODE == 2) { for (uint32_t i = threadIdx.x; i < n_iv; i += GW_THREADS) s_iv[i] = a.own_iv[i]; }
    if (threadIdx.x < 2) s_red[threadIdx.x] = 0;
    pdl_sync();
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1);
    const uint32_t gw = blockIdx.x * GW_WAVES + tid / PDL_WAVE;
    const uint32_t n = (uint32_t) scan_count(a.n_bound, a.d_n);
    const uint32_t tiles = (n + GW_TILE - 1) / GW_TILE;
    uint32_t n_rec = 0, n_grp = 0, n_rep = 0;
    for (uint32_t tile = gw; tile < tiles; tile += gridDim.x * GW_WAVES)
        gt_count_tile<MODE, false, LEAN>(a, tile, n, lane, s_iv, n_iv, nullptr, n_rec, n_grp, n_rep);
    gt_flush_counts<true>(a, s_red, n_rec, n_grp, n_rep);
}

// ---- the ranges sorted by gene without being written in record order first -------------------------------------------------
// (upper ranges for every gene, packed: the single-GPU build.)  The first radix pass of the gene sort would read what the
// write pass has just written; here the kernel that BUILDS the ranges is that pass: a workgroup takes PDL_RADIX_TILE = 4
// tiles of records, k_range_count_hist has counted its ranges by the low byte of their gene (the pass's histogram; a record
// that gets no range is simply not there), the scan of those counts says where every (block, byte) run starts, and
// k_range_scatter makes the ranges as k_group_write<1> does and files them as k_rs_scatter does (ballot ranks, digit-sorted
// in LDS, coalesced runs out).  Saves the ranges' trip through HBM (12 B written + 16 B read per range) and three launches.
static_assert(GW_WAVES * GW_TILE == (int) PDL_RADIX_TILE && GW_THREADS == (int) PDL_RADIX_BINS, "a workgroup's four tiles are one tile of the radix pass");
template <bool LEAN>
__global__ __launch_bounds__(GW_THREADS) void k_range_count_hist(GroupTileArgs a, uint32_t n_tiles4, uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_h[PDL_RADIX_BINS];
    __shared__ uint32_t s_red[2];
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
    const uint32_t n = (uint32_t) scan_count(a.n_bound, a.d_n);
    if (tid < 2) s_red[tid] = 0;
    uint32_t n_rec = 0, n_grp = 0, n_rep = 0;
    for (uint32_t blk = blockIdx.x; blk < n_tiles4; blk += gridDim.x) {       // (uniform loop: barriers inside)
        s_h[tid] = 0;
        pdl_sync();
        const uint32_t tile = blk * GW_WAVES + wave;
        if (tile * GW_TILE < n) gt_count_tile<1, true, LEAN>(a, tile, n, lane, nullptr, 0u, s_h, n_rec, n_grp, n_rep);      // (wave-uniform)
        pdl_sync();
        counts[(size_t) tid * n_tiles4 + blk] = s_h[tid];
    }
    gt_flush_counts<true>(a, s_red, n_rec, n_grp, n_rep);
}

// ---- write ---------------------------------------------------------------------------------------------------------------------
// One WAVE per tile, as in the costs kernel.  The ranges of a tile go to (scanned total of the 64-tile blocks before) +
// (tiles before it in its block) + rank inside the tile, i.e. in record order: the gene as sort key and the 16-byte tuple
// {first posting, postings, own count, group size} or the packed range.  In the upper modes the last member of a group has
// no range of its own: its group's size is added to its gene's cost here (tuples; packed ranges: costs are made on demand).
template <int MODE>
__global__ __launch_bounds__(GW_THREADS) void k_group_write(GroupTileArgs a) {
    extern __shared__ unsigned long long s_dyn[];        // shard modes: the intervals
    __shared__ unsigned long long s_own;
    uint2 *s_iv = reinterpret_cast<uint2 *>(s_dyn);
    const uint32_t n_iv = (MODE == 0 || MODE == 2) ? a.n_own_iv : 0u;
    if constexpr (MODE == 0 || MODE == 2) { for (uint32_t i = threadIdx.x; i < n_iv; i += GW_THREADS) s_iv[i] = a.own_iv[i]; }
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1);
    const uint32_t gw = blockIdx.x * GW_WAVES + tid / PDL_WAVE;
    const uint32_t n = (uint32_t) scan_count(a.n_bound, a.d_n);
    const uint32_t tiles = (n + GW_TILE - 1) / GW_TILE;
    if (tid == 0) s_own = 0;
    pdl_sync();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned long long own_lookups = 0;
    for (uint32_t tile = gw; tile < tiles; tile += gridDim.x * GW_WAVES) {
        const uint32_t t0 = tile * GW_TILE;
        uint2 po[GW_ROUNDS];
        gt_load_tile(a.post, t0, n, lane, po);
        uint32_t hb, ha;
        gt_load_borders(a, tile, tiles, lane, hb, ha);
        const uint32_t ins = gt_shard_mask<MODE>(a, s_iv, n_iv, po);
        unsigned long long m[GW_ROUNDS];
        gt_head_masks(po, t0, n, lane, m);
        uint32_t before, after;
        gt_tile_borders(a, tile, tiles, t0, n, m[0], lane, hb, ha, before, after);
        uint32_t nextr[GW_ROUNDS];
        gt_next_heads(m, t0, after, nextr);
        uint32_t pr = before, cnt_tile = 0;              // (uniform) last head before the current round; ranges so far in the tile
        const uint32_t tile_prefix = a.chunk_sums[tile / PDL_WAVE] + a.tile_sums[tile];
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) {
            const uint32_t u = t0 + j * PDL_WAVE + lane;
            uint32_t gs, ge;
            gt_round_extent(m[j], t0 + j * PDL_WAVE, lane, nextr[j], pr, gs, ge);
            const bool live = u < n;
            const bool shared = live && ge - gs >= 2;
            const bool mine = MODE == 1 || ((ins >> j) & 1u);
            bool r = shared && mine;
            if constexpr (MODE == 1 || MODE == 2) r = r && u + 1 < ge;           // the last member of a group has nothing above it
            const unsigned long long rb = __ballot(r);
            const uint32_t cnt = gt_take_head(a, tile, j, po[j].y, m[j], lane);
            if (live) {
                if (shared && mine) own_lookups += ge - gs;
                if (r) {
                    const uint32_t at = tile_prefix + cnt_tile + (uint32_t) __popcll(rb & lt_mask);
                    const uint32_t start = MODE == 0 ? gs : u + 1;
                    a.key2[at] = po[j].x;
                    if (a.pay8) a.pay8[at] = gt_pack_range(start, ge - start, cnt, a.pos_base);
                    else a.tuples[at] = make_uint4(start, ge - start, cnt, ge - gs);     // {first posting, postings, own count, group size}
                } else if (MODE == 1 || MODE == 2) {
                    if (!a.pay8 && ge - gs >= 2 && u + 1 == ge && mine) atomicAdd(&a.cost[po[j].x], (unsigned long long) (ge - gs));
                }
            }
            cnt_tile += (uint32_t) __popcll(rb);
        }
    }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) own_lookups += __shfl_xor(own_lookups, d, PDL_WAVE);
    if (lane == 0 && own_lookups) atomicAdd(&s_own, own_lookups);
    pdl_sync();
    if (tid == 0 && s_own) atomicAdd(&a.counters[2], s_own);
}

__global__ __launch_bounds__(GW_THREADS) void k_range_scatter(GroupTileArgs a, uint32_t n_tiles4, const uint32_t *__restrict__ offs,
                                                              uint32_t *__restrict__ keys_out, unsigned long long *__restrict__ vals_out,
                                                              const uint32_t *__restrict__ digit_total, uint64_t *d_total) {      // offsets one row per digit: see radix_tile_scan
    const uint32_t n = (uint32_t) scan_count(a.n_bound, a.d_n);
    if ((uint64_t) blockIdx.x * PDL_RADIX_TILE >= n) {                     // (uniform) block past the end
        if (digit_total && blockIdx.x == 0 && threadIdx.x == 0) *d_total = 0;      // (no records: no ranges)
        return;
    }
    __shared__ RadixTileLds<uint32_t, unsigned long long, uint16_t> s;      // (16-bit counters: three workgroups per CU)
    __shared__ unsigned long long s_own;
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
    const uint32_t tiles = (n + GW_TILE - 1) / GW_TILE;
    const uint32_t tile = blockIdx.x * GW_WAVES + wave, t0 = tile * GW_TILE;
    const bool active = tile < tiles;                    // (wave-uniform; the last block may hold fewer than four tiles)
    s.clear_counts();
    const uint32_t goff = offs[(size_t) tid * n_tiles4 + blockIdx.x];
    const uint32_t dtot = digit_total ? digit_total[tid] : 0u;
    if (tid == 0) s_own = 0;
    pdl_sync();

    uint2 po[GW_ROUNDS];
    unsigned long long val[GW_ROUNDS];
    uint16_t rank[GW_ROUNDS];
    uint32_t rbits = 0;                                  // bit j: this lane's record of round j gets a range
    unsigned long long own_lookups = 0;
    gt_load_tile(a.post, t0, n, lane, po);
    if (active) {
        uint32_t hb, ha;
        gt_load_borders(a, tile, tiles, lane, hb, ha);
        unsigned long long m[GW_ROUNDS];
        gt_head_masks(po, t0, n, lane, m);
        uint32_t before, after;
        gt_tile_borders(a, tile, tiles, t0, n, m[0], lane, hb, ha, before, after);
        uint32_t nextr[GW_ROUNDS];
        gt_next_heads(m, t0, after, nextr);
        uint32_t pr = before;
#pragma unroll
        for (int j = 0; j < GW_ROUNDS; j++) {
            const uint32_t u = t0 + j * PDL_WAVE + lane;
            uint32_t gs, ge;
            gt_round_extent(m[j], t0 + j * PDL_WAVE, lane, nextr[j], pr, gs, ge);
            const bool live = u < n;
            const bool shared = live && ge - gs >= 2;
            const bool r = shared && u + 1 < ge;         // the last member of a group has nothing above it
            const uint32_t cnt = gt_take_head(a, tile, j, po[j].y, m[j], lane);
            if (shared) own_lookups += ge - gs;
            val[j] = gt_pack_range(u + 1, ge - u - 1, cnt, 0u);
            rbits |= (uint32_t) r << j;
        }
    }
    // ---- the radix pass on the low byte of the gene (the tile body of pdl_sort.h; an element is a record with a range) ------
    uint32_t key[GW_ROUNDS];
#pragma unroll
    for (int j = 0; j < GW_ROUNDS; j++) key[j] = po[j].x;
    const auto valid = [&](int j) { return (rbits >> j) & 1u; };
    radix_rank_rounds<8>(s.cnt[wave], key, 0u, valid, rank);
    pdl_sync();
    uint32_t grand_total;
    const uint32_t tile_total = radix_tile_layout(s, goff, dtot, grand_total);       // (offsets from the three-launch scan: no digit totals, base 0)
    if (digit_total && blockIdx.x == 0 && tid == 0) *d_total = grand_total;
    pdl_sync();
    radix_tile_place(s, wave, key, val, 0u, valid, rank);
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) own_lookups += __shfl_xor(own_lookups, d, PDL_WAVE);
    if (lane == 0 && own_lookups) atomicAdd(&s_own, own_lookups);
    pdl_sync();
    radix_tile_write(s, 0u, tile_total, keys_out, vals_out);
    if (tid == 0 && s_own) atomicAdd(&a.counters[2], s_own);
}

// Between the passes: tile_sums[t] (ranges of tile t) becomes the count of the tiles before t inside its block of 64 tiles,
// chunk_sums[b] the block's total (scanned next); one wave per block.
__global__ __launch_bounds__(256) void k_tile_prefix(uint32_t *__restrict__ tile_sums, const uint64_t *d_n, uint64_t n_bound,
                                                     uint32_t *__restrict__ chunk_sums, uint32_t n_blocks) {
    const uint32_t b = blockIdx.x * 4 + threadIdx.x / PDL_WAVE, lane = threadIdx.x & (PDL_WAVE - 1);
    if (b >= n_blocks) return;
    const uint32_t tiles = (uint32_t) ((scan_count(n_bound, d_n) + GW_TILE - 1) / GW_TILE);
    const uint32_t t = b * PDL_WAVE + lane;
    const uint32_t v = t < tiles ? tile_sums[t] : 0u;
    const uint32_t inc = wave_inclusive_scan_u32(v);
    if (t < tiles) tile_sums[t] = inc - v;
    if (lane == PDL_WAVE - 1) chunk_sums[b] = inc;
}

// ---- launch helpers --------------------------------------------------------------------------------------------------------
// The planned arguments of a pass over `bound` postings at most (their count at d_n, or — nullptr — the bound itself) and its grid: the
// scratch of the count / write pair (tile_sums[tiles] | th_first[tiles] | th_last[tiles] | chunk_sums[blocks of 64 tiles]) and the genome
// of every gene.  What the callers differ by they set themselves: counters, cost, g_full / g_upper, pos_base, the shard.
struct GroupPlan { GroupTileArgs a; uint32_t grid; };
static GroupPlan group_tiles_plan(pdl_ctx *c, uint2 *post, uint64_t bound, const uint64_t *d_n) {
    const uint64_t tiles = (bound + GW_TILE - 1) / GW_TILE;
    if (tiles > 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "dictionary of %llu records exceeds the grid limit", (unsigned long long) bound);
    GroupPlan p{}; GroupTileArgs &a = p.a;
    a.post = post; a.n_bound = bound; a.d_n = d_n;
    a.n_blocks = (uint32_t) ((tiles + PDL_WAVE - 1) / PDL_WAVE);
    p.grid = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((tiles + GW_WAVES - 1) / GW_WAVES, (uint64_t) pdl_cus(c) * 8));
    c->scan_tmp.alloc(((size_t) tiles * 3 + a.n_blocks + 1) * sizeof(uint32_t));
    a.tile_sums = c->scan_tmp.as<uint32_t>(); a.th_first = a.tile_sums + tiles; a.th_last = a.th_first + tiles; a.chunk_sums = a.th_last + tiles;
    a.genome_of = c->d_gen; a.n_genomes = c->G;
    return p;
}
template <bool GENOMES, bool RECORD_COSTS>
static void launch_group_costs(pdl_ctx *c, const GroupTileArgs &a, uint32_t grid) {
    const size_t dyn = GENOMES && a.n_genomes <= COST_LDS_GENOMES ? 2 * (size_t) a.n_genomes * sizeof(uint64_t) : 0;
    hipLaunchKernelGGL((k_group_costs<GENOMES, RECORD_COSTS>), dim3(grid), dim3(GW_THREADS), dyn, c->stream, a);
    PDL_HIP(hipGetLastError());
}
// f(std::integral_constant<int, MODE>) for a range mode given at run time
template <class F>
static void with_range_mode(int mode, F &&f) {
    if (mode == 1) f(std::integral_constant<int, 1>{});
    else if (mode == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
// count + the scan of the tile counts; their total (the ranges the write pass will make) lands in scalars[PDL_CTL_RANGES]
static void launch_range_count(pdl_ctx *c, const GroupTileArgs &a, uint32_t grid, int mode) {
    const size_t dyn = (size_t) a.n_own_iv * sizeof(uint2);      // (mode 1: no shard, no intervals)
    with_range_mode(mode, [&](auto m) {
        if (c->opt_lean_records) hipLaunchKernelGGL((k_range_count<decltype(m)::value, true>), dim3(grid), dim3(GW_THREADS), dyn, c->stream, a);
        else hipLaunchKernelGGL((k_range_count<decltype(m)::value, false>), dim3(grid), dim3(GW_THREADS), dyn, c->stream, a);
    });
    hipLaunchKernelGGL(k_tile_prefix, dim3((a.n_blocks + 3) / 4), dim3(256), 0, c->stream, a.tile_sums, a.d_n, a.n_bound, a.chunk_sums, a.n_blocks);
    launch_tile_scan(c, a.chunk_sums, a.n_blocks, c->scalars.as<uint64_t>() + PDL_CTL_RANGES, nullptr);
    PDL_HIP(hipGetLastError());
}
static void launch_range_write(pdl_ctx *c, const GroupTileArgs &a, uint32_t grid, int mode) {
    const size_t dyn = (size_t) a.n_own_iv * sizeof(uint2);
    with_range_mode(mode, [&](auto m) { hipLaunchKernelGGL(k_group_write<decltype(m)::value>, dim3(grid), dim3(GW_THREADS), dyn, c->stream, a); });
    PDL_HIP(hipGetLastError());
}
