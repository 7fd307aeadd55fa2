// pdl_dict.hip — the dictionary stage on the device: everything preprocessSequences does
// (ig/native/library.cpp:189-371), one kernel (or kernel group) per reference function:
//
//   K-hist    k_hist              alphabet (which letters occur)             library.cpp:216-228
//   (host)    rank_init_host      rank table, B^(k-1), overflow -> hashing   library.cpp:88-132   (pdl_rekey.h, host section)
//   K-len     k_kseq_len          kseq_lengths + k-mer stream offsets        library.cpp:250-262
//   K-rank    k_rank / k_rank_hash   per-gene k-mer ranks                    library.cpp:75-86,134-150
//   K-sort    pdl_sort_pairs      stable LSD radix sort by rank              library.cpp:172-187,270-278
//   K-rle     k_rle_tile_sums / k_rle_apply (or RecHead/RecScatter through the generic scan)   dedup -> (rank,gene,count)   library.cpp:280-287
//   K-groups  k_fold_last_record, then per tile from the head bits: costs / count / write (pdl_groups.h)   library.cpp:297-335
//   K-ranges  k_group_write or k_range_scatter (ranges), sort by gene, k_gather_ranges (+ per-gene cost), k_seq_offsets   library.cpp:312-327
//   K-cost    k_genome_cost       per-genome and total lookups               library.cpp:337-350,535-538
//   (option "alphabet_rekey": k_short_letters, pdl_rekey.h — the letters of genes shorter than k, per genome; no reference function)
//
// HBM layout after this stage (what the join reads):
//   post   uint2[U]   {gene, count}       rank-group major, ascending gene inside a group
//   ranges uint4[U']  {first posting, postings, own count, group size}   gene major (U' = records in groups >= 2);
//                     without a shard a gene's range holds only the postings after its own record (genes above it)
//   seq_off u32[N+1]  range list of each gene;   kseq_len u32[N];   cost u64[N]
//
// K-append and K-remove share their host side: rk_change (the alphabet decision, pdl_rekey.h), commit_set_change,
// genome_ids_on_device, rekey_in_place and the tail rebuild_behind_sort; the key width picks a template through pdl_with_key.
#include "pdl_common.h"
#include "pdl_scan.h"
#include "pdl_sort.h"
#include "pdl_append.h"
#include "pdl_remove.h"
#include "pdl_rekey.h"
#include "pdl_groups.h"

#include <algorithm>
#include <cstring>


__global__ __launch_bounds__(256) void k_zero_u64(uint64_t *p, size_t n) {
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256) p[i] = 0;
}
// ------------------------------------------------------------------------------------------------
// K-hist: which byte values occur among the residues (library.cpp:216-228).  The reference counts every letter, but the
// counters are only ever asked "> 0?" (rank_init, library.cpp:96-99): the alphabet is a 256-entry presence table.  That
// needs no atomic anywhere: a lane stores a 1 into the LDS word of each byte it sees (lanes that meet the same letter store
// the same value to the same address; ~20 distinct letters fall in as many banks), and a workgroup stores a 1 into the
// global counter of every letter it has seen (same value from every workgroup).  16-byte coalesced loads, four in flight
// per lane: the pass runs at the speed the residues stream in (the counting version — LDS atomics on ~20 hot addresses —
// took 41 us for 17.6 MB).
// ------------------------------------------------------------------------------------------------
constexpr int HIST_THREADS = 256;
__global__ __launch_bounds__(HIST_THREADS) void k_hist(const uint8_t *__restrict__ res, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t s_seen[256];
    s_seen[threadIdx.x] = 0;
    pdl_sync();
    const uint64_t n16 = n / 16;
    const uint4 *res16 = reinterpret_cast<const uint4 *>(res);
    const uint64_t stride = (uint64_t) gridDim.x * HIST_THREADS;
    auto mark = [&](const uint4 &v) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s_seen[w[j] & 0xff] = 1u; s_seen[(w[j] >> 8) & 0xff] = 1u; s_seen[(w[j] >> 16) & 0xff] = 1u; s_seen[w[j] >> 24] = 1u;
        }
    };
    uint64_t i = (uint64_t) blockIdx.x * HIST_THREADS + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 v0 = res16[i], v1 = res16[i + stride], v2 = res16[i + 2 * stride], v3 = res16[i + 3 * stride];
        mark(v0); mark(v1); mark(v2); mark(v3);
    }
    for (; i < n16; i += stride) mark(res16[i]);
    if (blockIdx.x == 0)    // tail bytes
        for (uint64_t t = n16 * 16 + threadIdx.x; t < n; t += HIST_THREADS) s_seen[res[t]] = 1u;
    pdl_sync();
    if (s_seen[threadIdx.x]) hist[threadIdx.x] = 1ull;
}

// ------------------------------------------------------------------------------------------------
// K-len: kseq_lengths (library.cpp:250-262).  The exclusive scan of these is the offset of each
// gene in the k-mer stream (gene order = the order the reference emplace_back()s them, :255-258).
// ------------------------------------------------------------------------------------------------
struct KseqFlag {
    const uint64_t *off; uint32_t k;
    __device__ uint32_t operator()(uint64_t i) const {
        const uint64_t b = off[i], e = off[i + 1];
        const uint64_t len = e >= b ? e - b : 0;        // (descending offsets are reported by KseqApply)
        return len >= k ? (uint32_t) (len - k + 1) : 0u;
    }
};
struct KseqApply {
    uint32_t *kseq_len; uint32_t *gene_len; uint64_t *kmer_off;   // kmer_off as u64 for the API; values < 2^32 (checked on the host)
    unsigned long long *cost;                 // total_visited starts at zero (spares a fill)
    const uint64_t *off; uint64_t n_res; unsigned long long *bad;    // *bad |= 1 when the offsets are not an ascending cover of [0, n_res]
    __device__ void operator()(uint64_t i, uint32_t f, uint32_t prefix) const {
        kseq_len[i] = f;
        gene_len[i] = (uint32_t) (off[i + 1] - off[i]);        // (what kseq_len forgets of a gene shorter than k: pdl_remove_genomes' residue count)
        kmer_off[i] = prefix;
        cost[i] = 0;
        if (off[i + 1] < off[i] || off[i + 1] > n_res) atomicOr(bad, 1ull);     // (never taken on valid input)
    }
};

// K-len in ONE launch (option "fused_glue" n > 1, up to KL_MAX_GENES genes), after k_order_offsets: a workgroup owns KL_TILE genes, adds up
// the k-mer counts of the genes in front of them itself (the offsets are L2-resident: 8 bytes a gene) and scans its own, four
// consecutive genes per thread.  Nobody waits for another workgroup.  It writes what KseqFlag / KseqApply write, and clears the
// control block first (the k_zero_u64 in front of the scan): every workgroup a slice of it, except the two words this launch
// writes itself — the last workgroup, which has seen every offset, stores the total (PDL_CTL_KMERS, kmer_off[N]) and whether the
// offsets fail to ascend to the residue count (PDL_CTL_BAD_OFFSETS), plainly, so neither word needs to be zero beforehand.
constexpr uint32_t KL_THREADS = 1024, KL_ITEMS = 4, KL_TILE = KL_THREADS * KL_ITEMS;
// Measured: 14.1 / 19.4 / 30.0 / 53.0 us at 2^15 / 2^16 / 2^17 / 2^18 genes against 13.3 - 15.6 us for the clearing
// launch and the scan's kernels together — never below them, so "fused_glue" 1 leaves K-len its scan and only a value n > 1 asks
// for this kernel, for up to min(n, KL_MAX_GENES) genes.  The bound: up to 2^16 genes the one launch still ends sooner than the
// three it replaces (19.4 us against 21.8 from the first's start to the last's end); the last workgroup's read of everything in
// front of it doubles with the gene count, the scan's tiles do not.
constexpr uint32_t KL_MAX_GENES = 1u << 16;
struct KlenArgs {
    const uint64_t *off; uint64_t n_res; uint32_t k, n;
    uint32_t *kseq_len, *gene_len; uint64_t *kmer_off; unsigned long long *cost;
    uint64_t *ctl; uint64_t ctl_words;
};
__device__ __forceinline__ uint32_t kseq_of(uint64_t b, uint64_t e, uint32_t k) {
    const uint64_t len = e >= b ? e - b : 0;
    return len >= k ? (uint32_t) (len - k + 1) : 0u;
}
__global__ __launch_bounds__(KL_THREADS) void k_kseq_lengths(KlenArgs a) {
    constexpr uint32_t NW = KL_THREADS / PDL_WAVE;
    __shared__ unsigned long long s_sum[NW], s_front[NW];
    __shared__ uint32_t s_bad[NW];
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
    for (uint64_t i = (uint64_t) blockIdx.x * KL_THREADS + tid; i < a.ctl_words; i += (uint64_t) gridDim.x * KL_THREADS)
        if (i != PDL_CTL_KMERS && i != PDL_CTL_BAD_OFFSETS) a.ctl[i] = 0;
    const uint32_t r0 = min(blockIdx.x * KL_TILE, a.n), r1 = min(r0 + KL_TILE, a.n);
    // five offsets of four consecutive genes (from a multiple of four on: `off` is 16-byte aligned, the host has seen to that) in
    // three independent loads; the genes' k-mers summed, and whether an offset is out of order
    auto four = [&](uint32_t i, uint32_t *f4, uint32_t *gl4) -> uint32_t {
        const ulonglong2 lo = *reinterpret_cast<const ulonglong2 *>(a.off + i), hi = *reinterpret_cast<const ulonglong2 *>(a.off + i + 2);
        const uint64_t o[5] = {lo.x, lo.y, hi.x, hi.y, a.off[i + 4]};
        uint32_t wrong = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            f4[j] = kseq_of(o[j], o[j + 1], a.k); gl4[j] = (uint32_t) (o[j + 1] - o[j]);
            wrong |= (o[j + 1] < o[j] || o[j + 1] > a.n_res) ? 1u : 0u;
        }
        return wrong;
    };
    // the genes in front (r0 is a multiple of KL_TILE): their k-mers, and (of use to the last workgroup only) whether their
    // offsets are in order.  Eight trips' loads in flight: one at a time, each waited for, is all latency (57 us for 2^17 genes).
    unsigned long long front = 0;
    uint32_t bad = 0;
#pragma unroll 8
    for (uint32_t i = tid * KL_ITEMS; i < r0; i += KL_TILE) {
        uint32_t f4[4], gl4[4];
        bad |= four(i, f4, gl4);
        front += (unsigned long long) f4[0] + f4[1] + f4[2] + f4[3];
    }
    // this workgroup's genes
    const uint32_t i0 = r0 + tid * KL_ITEMS;
    uint32_t f[KL_ITEMS], gl[KL_ITEMS];
    unsigned long long sum = 0;
    if (i0 + KL_ITEMS <= r1) bad |= four(i0, f, gl);
    else {
#pragma unroll
        for (uint32_t j = 0; j < KL_ITEMS; j++) {
            f[j] = 0; gl[j] = 0;
            if (i0 + j < r1) {
                const uint64_t b = a.off[i0 + j], e = a.off[i0 + j + 1];
                f[j] = kseq_of(b, e, a.k); gl[j] = (uint32_t) (e - b);
                bad |= (e < b || e > a.n_res) ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < KL_ITEMS; j++) sum += f[j];
    unsigned long long inc = sum;
#pragma unroll
    for (int d = 1; d < PDL_WAVE; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, PDL_WAVE);
        if (lane >= (uint32_t) d) inc += o;
    }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) { front += __shfl_xor(front, d, PDL_WAVE); bad |= (uint32_t) __shfl_xor((int) bad, d, PDL_WAVE); }
    if (lane == PDL_WAVE - 1) s_sum[wave] = inc;
    if (lane == 0) { s_front[wave] = front; s_bad[wave] = bad; }
    pdl_sync();
    unsigned long long ex = inc - sum, total = 0;          // exclusive inside the wave, + the waves before, + the genes in front
    uint32_t bad_all = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; w++) {
        const unsigned long long v = s_sum[w], fr = s_front[w];
        ex += fr + (w < wave ? v : 0ull); total += fr + v; bad_all |= s_bad[w];
    }
#pragma unroll
    for (uint32_t j = 0; j < KL_ITEMS; j++) {
        if (i0 + j < r1) { a.kseq_len[i0 + j] = f[j]; a.gene_len[i0 + j] = gl[j]; a.kmer_off[i0 + j] = ex; a.cost[i0 + j] = 0; }
        ex += f[j];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) { a.ctl[PDL_CTL_KMERS] = total; a.kmer_off[a.n] = total; a.ctl[PDL_CTL_BAD_OFFSETS] = bad_all ? 1ull : 0ull; }
}

// ------------------------------------------------------------------------------------------------
// K-rank (exact): one thread per k-mer of the stream.  Because B^k < 2^64 here, the reference's
// rolling update (library.cpp:75-79) equals the direct base-B polynomial of the k residues, so
// k-mers are independent.  A workgroup covers RANK_TILE consecutive stream slots; two lanes
// bracket the genes of the tile with a binary search, every lane then searches only that bracket.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RANK_SPAN = 128;     // genes whose offsets a tile stages in LDS (more: global lookups)
constexpr int RANK_THREADS = 256;
constexpr int RANK_ITEMS = 4;
constexpr int RANK_TILE = RANK_THREADS * RANK_ITEMS;

__device__ __forceinline__ uint32_t upper_bound_u64(const uint64_t *a, uint32_t lo, uint32_t hi, uint64_t v) {
    // first index in [lo,hi) with a[idx] > v
    while (lo < hi) {
        uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct __attribute__((packed, aligned(1))) UnalignedU64 { uint64_t v; };
// eight residues from byte position p (any alignment); near the end of the buffer byte by byte
__device__ __forceinline__ uint64_t load_residues8(const uint8_t *__restrict__ res, uint64_t p, uint64_t n_res) {
    if (p + 8 <= n_res) return reinterpret_cast<const UnalignedU64 *>(res + p)->v;
    uint64_t w = 0;
    for (uint32_t b = 0; b < 8 && p + b < n_res; b++) w |= (uint64_t) res[p + b] << (8 * b);
    return w;
}

// Interval histogram of the multi-GPU build: the rank space is cut where the top DIST_BIN_BITS bits of a rank change.
constexpr uint32_t DIST_BIN_BITS = 12, DIST_BINS = 1u << DIST_BIN_BITS;

// upper_bound_u64 by a whole wave (all 64 lanes active, same arguments; every lane returns the same index): lane i probes one
// of 64 evenly spaced entries, a ballot picks the segment — three dependent loads for up to 64^3 entries where one lane's
// binary search makes eighteen.
__device__ __forceinline__ uint32_t wave_upper_bound_u64(const uint64_t *a, uint32_t lo, uint32_t hi, uint64_t v) {
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    // invariant: a[i] <= v for every i < lo, a[i] > v for every i >= hi
    while (hi - lo > PDL_WAVE) {
        const uint32_t step = (hi - lo + PDL_WAVE - 1) / PDL_WAVE;
        const uint64_t at = (uint64_t) lo + (uint64_t) lane * step;
        const bool le = at < hi && a[at] <= v;
        const uint32_t c = (uint32_t) __popcll(__ballot(le));        // (a ascends: the lanes 0 .. c-1)
        if (c == 0) return lo;
        const uint64_t next = (uint64_t) lo + (uint64_t) c * step;   // first probe above v, if it was made
        if (next < hi) hi = (uint32_t) next;
        lo = lo + (c - 1) * step + 1;
    }
    const bool le = lo + lane < hi && a[lo + lane] <= v;
    return lo + (uint32_t) __popcll(__ballot(le));
}

// MODE 0: keys[q] = rank, vals[q] = gene for every slot q of the k-mer stream (one workgroup per tile).
// MODE 1: the same, and counts the ranks by their top bits into bins[DIST_BINS] (persistent workgroups over the tiles,
//         LDS histogram, one global atomic per non-empty bin and workgroup): the k-mer count of every rank interval,
//         from which pdl_dist_preprocess_begin derives the same cuts on every GPU.
// MODE 2: as MODE 0, and files the first histogram of the rank sort: a workgroup covers one tile of the radix pass
//         (PDL_RADIX_TILE slots, in trips of RANK_TILE; its genes are bracketed and staged once), counts the low byte of the
//         ranks it writes and stores bins[byte * tiles + tile] — what k_rs_hist would count from the keys read back.
template <class KeyT, int MODE>
__global__ __launch_bounds__(RANK_THREADS) void k_rank(const uint8_t *__restrict__ res, const uint64_t *__restrict__ off,
                                                       const uint64_t *__restrict__ kmer_off, uint32_t n_seq, uint64_t m, uint64_t n_res,
                                                       RankParams rp, KeyT *__restrict__ keys, uint32_t *__restrict__ vals,
                                                       uint32_t bin_shift, uint32_t *__restrict__ bins) {
    static_assert(RANK_THREADS == (int) PDL_RADIX_BINS && PDL_RADIX_TILE % RANK_TILE == 0, "MODE 2: one thread per byte value, whole trips per radix tile");
    constexpr uint32_t TRIPS = MODE == 2 ? PDL_RADIX_TILE / RANK_TILE : 1;
    constexpr uint64_t TILE = (uint64_t) RANK_TILE * TRIPS;
    __shared__ uint8_t s_rv[256];
    __shared__ uint32_t s_lo, s_hi;
    __shared__ uint64_t s_koff[RANK_SPAN + 1], s_off[RANK_SPAN];    // k-mer and residue offsets of the genes this tile touches
    __shared__ uint32_t s_bins[MODE == 1 ? DIST_BINS : MODE == 2 ? PDL_RADIX_BINS : 1];
    for (int i = threadIdx.x; i < 256; i += RANK_THREADS) s_rv[i] = rp.rank_values[i];
    if constexpr (MODE == 1) for (uint32_t i = threadIdx.x; i < DIST_BINS; i += RANK_THREADS) s_bins[i] = 0;
    const uint64_t tiles = (m + TILE - 1) / TILE;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // MODE 0, 2: grid = tiles, one trip
    pdl_sync();                                            // (the staged boundaries of the previous tile are done with)
    const uint64_t q0 = tile * TILE;
    const uint64_t q_last = min(q0 + TILE, m) - 1;
    if (threadIdx.x < PDL_WAVE) {                          // (two whole waves, one bracket each)
        const uint32_t b = wave_upper_bound_u64(kmer_off, 0, n_seq + 1, q0) - 1;
        if (threadIdx.x == 0) s_lo = b;
    } else if (threadIdx.x < 2 * PDL_WAVE) {
        const uint32_t b = wave_upper_bound_u64(kmer_off, 0, n_seq + 1, q_last) - 1;
        if (threadIdx.x == PDL_WAVE) s_hi = b;
    }
    if constexpr (MODE == 2) s_bins[threadIdx.x] = 0;
    pdl_sync();
    const uint32_t lo = s_lo, hi = s_hi;
    const uint32_t span = hi - lo + 1;                          // genes under this tile (uniform)
    const bool staged = span <= RANK_SPAN;
    if (staged) {
        for (uint32_t i = threadIdx.x; i <= span; i += RANK_THREADS) s_koff[i] = kmer_off[lo + i];
        for (uint32_t i = threadIdx.x; i < span; i += RANK_THREADS) s_off[i] = off[lo + i];
    }
    pdl_sync();
    // (staged, at most 64 genes) the start of gene lo + lane; the lanes past the last gene hold the end of the bracket, above every slot of the tile
    const uint64_t my_koff = staged ? s_koff[min(threadIdx.x & (PDL_WAVE - 1), span)] : 0;
#pragma unroll 1
   for (uint32_t trip = 0; trip < TRIPS; trip++) {
    const uint64_t qt0 = q0 + (uint64_t) trip * RANK_TILE;
    if (qt0 >= m) break;                                        // (uniform; MODE 2: the stream's last tile)
    const uint32_t k = rp.k;
    const KeyT base = (KeyT) rp.base;                           // the polynomial fits KeyT (checked on the host): KeyT arithmetic
    // Phase 1: gene and residue position of the lane's four k-mers.  Phase 2: their residues, eight bytes per load, the
    // loads of the four k-mers in flight together (a byte loop with a wait per byte serialises 4 x k round trips).
    uint32_t sq[RANK_ITEMS];
    uint64_t pos[RANK_ITEMS];
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; j++) {
        const uint64_t qj = qt0 + (uint64_t) j * RANK_THREADS + threadIdx.x;
        const uint64_t q = qj < m ? qj : m - 1;
        if (staged) {                                           // (uniform) boundaries from LDS: no chain of global loads
            uint32_t a = 0;                                     // last i in [0, span) with s_koff[i] <= q
            if (span <= PDL_WAVE) {                             // (uniform, the usual case) lane i holds the start of gene lo + i: two ballots
                // bracket the genes under the wave's 64 consecutive slots, mostly one gene or two; the lane counts the starts between
                const uint64_t qf = min(qt0 + (uint64_t) j * RANK_THREADS + (threadIdx.x & ~(PDL_WAVE - 1)), m - 1), ql = min(qf + PDL_WAVE - 1, m - 1);
                const uint32_t a0 = (uint32_t) __popcll(__ballot(my_koff <= qf)) - 1, a1 = (uint32_t) __popcll(__ballot(my_koff <= ql)) - 1;
                a = a0;
                for (uint32_t i = a0 + 1; i <= a1; i++) a += (uint32_t) (s_koff[i] <= q);
            } else {
                uint32_t b = span;
                while (a < b) { const uint32_t mid = (a + b) >> 1; if (s_koff[mid + 1] <= q) a = mid + 1; else b = mid; }
            }
            sq[j] = lo + a;
            pos[j] = s_off[a] + (q - s_koff[a]);
        } else {
            sq[j] = upper_bound_u64(kmer_off, lo, hi + 1, q) - 1;   // kmer_off[s] <= q < kmer_off[s+1]
            pos[j] = off[sq[j]] + (q - kmer_off[sq[j]]);
        }
    }
    KeyT r[RANK_ITEMS];
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; j++) r[j] = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += 8) {
        uint64_t w[RANK_ITEMS];
        bool safe = true;
#pragma unroll
        for (int j = 0; j < RANK_ITEMS; j++) safe = safe && pos[j] + c0 + 8 <= n_res;
        if (__all(safe)) {                                      // (every tile but the last): four unaligned 8-byte loads, no branches between them
#pragma unroll
            for (int j = 0; j < RANK_ITEMS; j++) w[j] = reinterpret_cast<const UnalignedU64 *>(res + pos[j] + c0)->v;
        } else {
#pragma unroll
            for (int j = 0; j < RANK_ITEMS; j++) w[j] = load_residues8(res, pos[j] + c0, n_res);
        }
        const uint32_t nb = min(8u, k - c0);
        for (uint32_t b = 0; b < nb; b++) {
#pragma unroll
            for (int j = 0; j < RANK_ITEMS; j++) r[j] = r[j] * base + s_rv[(uint32_t) (w[j] >> (8 * b)) & 0xffu];
        }
    }
#pragma unroll
    for (int j = 0; j < RANK_ITEMS; j++) {
        const uint64_t q = qt0 + (uint64_t) j * RANK_THREADS + threadIdx.x;
        if (q < m) {
            if constexpr (MODE == 1) atomicAdd(&s_bins[(uint32_t) (r[j] >> bin_shift)], 1u);
            if constexpr (MODE == 2) atomicAdd(&s_bins[(uint32_t) r[j] & (PDL_RADIX_BINS - 1)], 1u);      // (the digit of k_rs_scatter's first pass)
            keys[q] = r[j]; vals[q] = sq[j];
        }
    }
   }
    if constexpr (MODE == 2) {
        pdl_sync();
        bins[(size_t) threadIdx.x * tiles + tile] = s_bins[threadIdx.x];
    }
  }
    if constexpr (MODE == 1) {
        pdl_sync();
        for (uint32_t i = threadIdx.x; i < DIST_BINS; i += RANK_THREADS) { const uint32_t v = s_bins[i]; if (v) atomicAdd(&bins[i], v); }
    }
}

// K-rank (hash fallback, library.cpp:81-86): the 64-bit wrap of the first line makes the value
// depend on the whole prefix of the gene, so genes are ranked sequentially, one lane per gene.
__device__ __forceinline__ uint64_t update_rank_hash_dev(uint64_t current, uint64_t vnext, uint64_t vpop, uint64_t lm, uint64_t base) {
    uint64_t wrapped = current + RABIN_MODULO - vpop * lm;       // evaluated in 64 bits, wraps
    // (wrapped * base + vnext) mod (2^64 - 59) with a 128-bit intermediate
    uint64_t lo = wrapped * base;
    uint64_t hi = __umul64hi(wrapped, base);
    uint64_t lo2 = lo + vnext;
    hi += (lo2 < lo);
    // hi * 2^64 + lo2  ==  hi * 59 + lo2   (mod 2^64 - 59); hi < 256 so hi*59 is tiny
    uint64_t t = hi * 59ull;
    uint64_t r = lo2 + t;
    if (r < lo2) r += 59ull;                                     // one more 2^64 folded (cannot carry again)
    if (r >= RABIN_MODULO) r -= RABIN_MODULO;
    return r;
}

// MODE 1 also counts the ranks by their top DIST_BIN_BITS bits (see k_rank).
template <int MODE>
__global__ __launch_bounds__(256) void k_rank_hash(const uint8_t *__restrict__ res, const uint64_t *__restrict__ off,
                                                   const uint64_t *__restrict__ kmer_off, uint32_t n_seq, RankParams rp,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ bins) {
    __shared__ uint8_t s_rv[256];
    for (int i = threadIdx.x; i < 256; i += 256) s_rv[i] = rp.rank_values[i];
    pdl_sync();
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seq) return;
    const uint64_t b = off[s], e = off[s + 1];
    const uint32_t k = rp.k;
    if (e - b < k) return;
    const uint8_t *p = res + b;
    const uint64_t len = e - b;
    uint64_t q = kmer_off[s];
    uint64_t rank = 0;
    const uint64_t v0 = s_rv[0];
    for (uint32_t i = 0; i < k; i++) rank = update_rank_hash_dev(rank, s_rv[p[i]], v0, rp.last_multiplier, rp.base);
    if constexpr (MODE == 1) atomicAdd(&bins[rank >> (64 - DIST_BIN_BITS)], 1u);
    keys[q] = rank; vals[q] = s; q++;
    for (uint64_t i = k; i < len; i++) {
        rank = update_rank_hash_dev(rank, s_rv[p[i]], s_rv[p[i - k]], rp.last_multiplier, rp.base);
        if constexpr (MODE == 1) atomicAdd(&bins[rank >> (64 - DIST_BIN_BITS)], 1u);
        keys[q] = rank; vals[q] = s; q++;
    }
}

// ------------------------------------------------------------------------------------------------
// K-rle: run-length dedup of the sorted stream (library.cpp:280-287).  A record head is a position
// whose (rank, gene) differs from its predecessor; recpos[u] = position of the u-th head, the run
// length to the next head is the k-mer's multiplicity in the gene.
// ------------------------------------------------------------------------------------------------
template <class KeyT> struct RecHead {
    const KeyT *keys; const uint32_t *vals;
    __device__ uint32_t operator()(uint64_t q) const {     // straight-line (no short-circuit): the loads of a thread's items overlap
        const uint64_t qp = q ? q - 1 : 0;
        const KeyT k0 = keys[q], k1 = keys[qp];
        const uint32_t v0 = vals[q], v1 = vals[qp];
        return (uint32_t) (q == 0) | (uint32_t) (k0 != k1) | (uint32_t) (v0 != v1);
    }
};
// The apply side also builds the record: post[u] = {gene, run length | HEAD_BIT when record u opens a rank-group}
// (its rank differs from the element just before it, which belongs to the previous record).  Runs are short (a k-mer
// repeated inside one gene), so the head walks its own run.
template <class KeyT> struct RecScatter {
    const KeyT *keys; const uint32_t *vals; uint64_t m;
    uint32_t *recpos; uint2 *post;
    struct Loaded { uint32_t val, run; uint8_t head; };
    __device__ Loaded load(uint64_t q, uint32_t) const {    // straight-line for the common run of one; the rare longer run loops
        const uint64_t qp = q ? q - 1 : 0, qn = q + 1 < m ? q + 1 : q;
        const KeyT key = keys[q], kprev = keys[qp], knext = keys[qn];
        const uint32_t val = vals[q], vnext = vals[qn];
        const bool head = q == 0 || kprev != key;
        uint64_t j = q + 1;
        if (j < m && knext == key && vnext == val) {
            j++;
            while (j < m && keys[j] == key && vals[j] == val) j++;
        }
        return Loaded{val, (uint32_t) (j - q), (uint8_t) (head ? 1 : 0)};
    }
    __device__ void store(uint64_t q, uint32_t f, uint32_t prefix, const Loaded &v) const {
        if (!f) return;
        recpos[prefix] = (uint32_t) q;
        post[prefix] = make_uint2(v.val, v.run | ((uint32_t) v.head << 31));
    }
};

// K-rle in kernels of its own (option "lean_records"): key and value of a k-mer are loaded ONCE per pass, where RecHead and
// RecScatter behind the generic scan load nine words per k-mer.  A wave owns RLE_ROUNDS x 64 consecutive k-mers and reads them
// 64 at a time (lane l, round j: k-mer w0 + 64 j + l — 256 contiguous bytes per load, and the heads of a round go out as one
// contiguous run of records; four consecutive k-mers per lane with 16-byte loads would split every store instruction into 64
// separate 8- and 4-byte pieces four records apart).  The predecessor's key and value come from the lane below by a DPP move,
// for lane 0 from lane 63 of the round before, for the wave's first k-mer from one extra load.  "My successor repeats me" needs
// no key: a lane keeps its eight head bits in one word, ONE DPP move hands down the word of the lane above, lane 63 takes lane
// 0's shifted by a round, and the k-mer behind the wave is one extra load
// compared with lane 63's.  The prefix of a head is (heads of the tiles, waves and rounds before: scalars) + mbcnt of its
// round's ballot: no flag and no prefix goes through LDS.  rle_wave_heads is the body both kernels share.
constexpr int RLE_ROUNDS = 8, RLE_WAVES = SCAN_THREADS / PDL_WAVE;
constexpr uint32_t RLE_SPAN = RLE_ROUNDS * PDL_WAVE, RLE_TILE = RLE_WAVES * RLE_SPAN;
static_assert(RLE_TILE == (uint32_t) SCAN_TILE, "K-rle's tile sums are scanned like any scan's");

__device__ __forceinline__ uint32_t wave_prev_key(uint32_t v, uint32_t first) { return wave_prev_u32(v, first); }
__device__ __forceinline__ uint64_t wave_prev_key(uint64_t v, uint64_t first) { return wave_prev_u64(v, first); }
__device__ __forceinline__ uint32_t lane63_of(uint32_t v) { return (uint32_t) __builtin_amdgcn_readlane((int) v, PDL_WAVE - 1); }
__device__ __forceinline__ uint64_t lane63_of(uint64_t v) { return (uint64_t) lane63_of((uint32_t) (v >> 32)) << 32 | lane63_of((uint32_t) v); }

// The wave's k-mers [w0, w0 + RLE_SPAN) of the m in the stream (w0 < m): key[j], val[j] of this lane's k-mer of round j (index
// clamped to m - 1), mh[j] = ballot of "is a record head" (false past m), heads = the lane's own bits of those (bit j: round j);
// returns bit j = the k-mer opens a rank-group.
template <class KeyT>
__device__ __forceinline__ uint32_t rle_wave_heads(const KeyT *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t w0, uint64_t m, uint32_t lane,
                                                   KeyT (&key)[RLE_ROUNDS], uint32_t (&val)[RLE_ROUNDS], unsigned long long (&mh)[RLE_ROUNDS], uint32_t &heads) {
    const uint32_t rem = (uint32_t) min(m - w0, (uint64_t) RLE_SPAN);            // live k-mers of the wave
    const uint64_t qp = w0 ? w0 - 1 : 0;
    KeyT kfirst = keys[qp];                                                      // the predecessor of the wave's first k-mer (uniform)
    uint32_t vfirst = vals[qp];
    const KeyT *kw = keys + w0;                                                  // (uniform bases, 32-bit lane offsets)
    const uint32_t *vw = vals + w0;
#pragma unroll
    for (int j = 0; j < RLE_ROUNDS; j++) {                                       // all loads first, branch-free
        const uint32_t e = j * PDL_WAVE + lane;
        const uint32_t ec = e < rem ? e : rem - 1;
        key[j] = kw[ec]; val[j] = vw[ec];
    }
    uint32_t rank_heads = 0;
    heads = 0;
#pragma unroll
    for (int j = 0; j < RLE_ROUNDS; j++) {
        const uint32_t e = j * PDL_WAVE + lane;
        const KeyT kprev = wave_prev_key(key[j], kfirst);
        const uint32_t vprev = wave_prev_u32(val[j], vfirst);
        const bool rank_head = (w0 == 0 && e == 0) || kprev != key[j];
        const bool head = e < rem && (rank_head || vprev != val[j]);
        mh[j] = __ballot(head);
        rank_heads |= (uint32_t) rank_head << j;
        heads |= (uint32_t) head << j;
        kfirst = lane63_of(key[j]); vfirst = lane63_of(val[j]);
    }
    return rank_heads;
}

template <class KeyT>
__global__ __launch_bounds__(SCAN_THREADS) void k_rle_tile_sums(const KeyT *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t m,
                                                                uint32_t *__restrict__ tile_sums) {
    __shared__ uint32_t s_wt[RLE_WAVES];
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1), wave = threadIdx.x / PDL_WAVE;
    const uint64_t w0 = (uint64_t) blockIdx.x * RLE_TILE + (uint64_t) wave * RLE_SPAN;
    uint32_t cnt = 0;
    if (w0 < m) {                                                                // (wave-uniform)
        KeyT key[RLE_ROUNDS]; uint32_t val[RLE_ROUNDS]; unsigned long long mh[RLE_ROUNDS];
        uint32_t heads;
        (void) rle_wave_heads(keys, vals, w0, m, lane, key, val, mh, heads);
#pragma unroll
        for (int j = 0; j < RLE_ROUNDS; j++) cnt += (uint32_t) __popcll(mh[j]);
    }
    if (lane == 0) s_wt[wave] = cnt;
    pdl_sync();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < RLE_WAVES; w++) total += s_wt[w];
        tile_sums[blockIdx.x] = total;
    }
}

// recpos[u] = position of record u's first k-mer, post[u] = {gene, run | head of a rank-group << 31}: what RecScatter writes.
// INLINE_PREFIX as in k_scan_apply: tile_sums holds the raw sums and the workgroup adds up the ones before its own.
template <class KeyT, bool INLINE_PREFIX>
__global__ __launch_bounds__(SCAN_THREADS) void k_rle_apply(const KeyT *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t m,
                                                            const uint32_t *__restrict__ tile_sums, uint32_t *__restrict__ recpos, uint2 *__restrict__ post,
                                                            uint64_t *d_total, uint64_t *d_total2) {
    __shared__ uint32_t s_wt[RLE_WAVES];
    __shared__ uint32_t s_wave[17];
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1), wave = threadIdx.x / PDL_WAVE;
    uint32_t tile_prefix = 0;
    if constexpr (INLINE_PREFIX) {
        const uint32_t upto = blockIdx.x == 0 ? gridDim.x : blockIdx.x;          // workgroup 0 adds up everything: the total
        uint32_t part = 0;
        for (uint32_t i = threadIdx.x; i < upto; i += SCAN_THREADS) part += tile_sums[i];
        uint32_t all;
        (void) block_exclusive_scan_u32(part, s_wave, all);
        if (blockIdx.x == 0) { if (threadIdx.x == 0) scan_write_totals(all, d_total, d_total2); }
        else tile_prefix = all;
    } else {
        tile_prefix = tile_sums[blockIdx.x];
    }
    const uint64_t w0 = (uint64_t) blockIdx.x * RLE_TILE + (uint64_t) wave * RLE_SPAN;
    const bool live_wave = w0 < m;                                               // (wave-uniform)
    KeyT key[RLE_ROUNDS]; uint32_t val[RLE_ROUNDS]; unsigned long long mh[RLE_ROUNDS];
    uint32_t rank_heads = 0, heads = 0, cnt = 0;
    bool last_repeats = false;                                                   // the k-mer behind the wave's last repeats it (uniform)
    if (live_wave) {
        const uint64_t qn = w0 + RLE_SPAN;
        const bool has_next = qn < m;
        const KeyT knext = keys[has_next ? qn : m - 1];
        const uint32_t vnext = vals[has_next ? qn : m - 1];
        rank_heads = rle_wave_heads(keys, vals, w0, m, lane, key, val, mh, heads);
        last_repeats = has_next && knext == lane63_of(key[RLE_ROUNDS - 1]) && vnext == lane63_of(val[RLE_ROUNDS - 1]);
#pragma unroll
        for (int j = 0; j < RLE_ROUNDS; j++) cnt += (uint32_t) __popcll(mh[j]);
    }
    if (lane == 0) s_wt[wave] = cnt;
    pdl_sync();
    if (!live_wave) return;
    uint32_t at0 = tile_prefix;                                                  // records before the wave's first k-mer
#pragma unroll
    for (int w = 0; w < RLE_WAVES; w++) at0 += w < (int) wave ? s_wt[w] : 0u;
    // bit j: the successor of this lane's k-mer of round j is a head — the lane above holds it; lane 63: lane 0's next round, or
    // the k-mer behind the wave — or the end of the stream
    const uint32_t first_heads = (uint32_t) __builtin_amdgcn_readfirstlane((int) heads);
    uint32_t next_heads = wave_next_u32(heads, first_heads >> 1 | (last_repeats ? 0u : 1u) << (RLE_ROUNDS - 1));
    const uint32_t remn = (uint32_t) min(m - w0, (uint64_t) RLE_SPAN + 1);       // k-mer e of the wave has a successor iff e + 1 < remn
    if (remn <= RLE_SPAN) {                                                      // (uniform) the stream ends in this wave
#pragma unroll
        for (int j = 0; j < RLE_ROUNDS; j++) next_heads |= (uint32_t) (j * PDL_WAVE + lane + 1 >= remn) << j;
    }
    uint32_t run[RLE_ROUNDS];
#pragma unroll
    for (int j = 0; j < RLE_ROUNDS; j++) run[j] = 1;
    const uint32_t walks = heads & ~next_heads;                                  // a k-mer repeated inside its gene: the head walks its run
    if (walks) {                                                                 // (rare; its loads stand before every store)
#pragma unroll
        for (int j = 0; j < RLE_ROUNDS; j++) {
            if ((walks >> j) & 1u) {
                const uint64_t q = w0 + j * PDL_WAVE + lane;
                uint64_t jx = q + 2;
                while (jx < m && keys[jx] == key[j] && vals[jx] == val[j]) jx++;
                run[j] = (uint32_t) (jx - q);
            }
        }
    }
    const uint32_t q0 = (uint32_t) w0 + lane;                                    // (stream positions fit 32 bits: recpos)
#pragma unroll
    for (int j = 0; j < RLE_ROUNDS; j++) {
        if ((heads >> j) & 1u) {
            const uint32_t at = at0 + __builtin_amdgcn_mbcnt_hi((uint32_t) (mh[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mh[j], 0u));
            recpos[at] = q0 + j * PDL_WAVE;
            post[at] = make_uint2(val[j], run[j] | ((rank_heads >> j) & 1u) << 31);
        }
        at0 += (uint32_t) __popcll(mh[j]);
    }
}

// Interval selection of the multi-GPU build: the k-mers whose rank falls into this GPU's bins, in stream order.
template <class KeyT> struct SelFlag {
    const KeyT *keys; uint32_t shift, b_lo, b_hi;
    __device__ uint32_t operator()(uint64_t q) const { const uint32_t b = (uint32_t) (keys[q] >> shift); return (uint32_t) (b >= b_lo) & (uint32_t) (b < b_hi); }
};
template <class KeyT> struct SelApply {
    const KeyT *keys; const uint32_t *vals; KeyT *keys_out; uint32_t *vals_out;
    struct Loaded { KeyT key; uint32_t val; };
    __device__ Loaded load(uint64_t q, uint32_t f) const { return f ? Loaded{keys[q], vals[q]} : Loaded{0, 0u}; }      // (seven k-mers in eight belong to other ranks: their key and gene are not read again)
    __device__ void store(uint64_t, uint32_t f, uint32_t prefix, const Loaded &v) const { if (f) { keys_out[prefix] = v.key; vals_out[prefix] = v.val; } }
};

// in_shard[gene] = the gene's genome belongs to this rank (multi-GPU: from the genome deal, without a host round trip)
__global__ __launch_bounds__(256) void k_genes_of_rank(const uint32_t *__restrict__ genome_of, const uint32_t *__restrict__ owner, uint32_t rank,
                                                       uint32_t n_seq, uint8_t *__restrict__ in_shard) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_seq) in_shard[s] = owner[genome_of[s]] == rank ? 1 : 0;
}
// seq_owner[gene] = rank that owns the gene's genome
__global__ __launch_bounds__(256) void k_gene_owner(const uint32_t *__restrict__ genome_of, const uint32_t *__restrict__ owner, uint32_t n_seq,
                                                    uint8_t *__restrict__ seq_owner) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_seq) seq_owner[s] = (uint8_t) owner[genome_of[s]];
}
// key = owner(gene) << 24 | gene: one radix pass on the top byte files the tuples by destination, in record order
__global__ __launch_bounds__(256) void k_owner_keys(uint32_t *__restrict__ key, const uint64_t *d_n, const uint8_t *__restrict__ seq_owner) {
    const uint32_t n = (uint32_t) *d_n;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t g = key[i];
        key[i] = g | ((uint32_t) seq_owner[g] << 24);
    }
}
// What a peer sent (pdl_dist_preprocess_finish_ranges), counted before any of it is sorted or used, as k_fam_check counts a caller's
// edges: a key that is not (this rank << 24 | a gene of this rank's genomes) — the gene sort promises pdl_sort_pairs that every gene
// lies below N — and a packed range (gt_pack_range) that reaches past the gathered dictionary.
__global__ __launch_bounds__(256) void k_tuple_check(const uint32_t *__restrict__ key, const unsigned long long *__restrict__ range, uint32_t n,
                                                     const uint8_t *__restrict__ seq_owner, uint32_t n_seq, uint32_t rank, uint32_t total, uint64_t *d_bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i], g = k & 0xffffffu;
    const unsigned long long r = range[i];
    const unsigned long long end = (r & 0xffffffffull) + ((r >> 32) & 0x3fffffull);       // first posting + postings
    if ((k >> 24) != rank || g >= n_seq || seq_owner[g] != rank || end > total) atomicAdd(reinterpret_cast<unsigned long long *>(d_bad), 1ull);
}

// Also adds up total_visited (library.cpp:327) = the group sizes over a gene's ranges: the list is gene-sorted, so a
// wave holds one or two genes as a rule; one atomic per (wave, gene).
__global__ __launch_bounds__(256) void k_gather_ranges(const uint32_t *__restrict__ idx_sorted, const uint32_t *__restrict__ key_sorted,
                                                       const uint4 *__restrict__ tuples, const uint64_t *d_n, uint4 *__restrict__ ranges,
                                                       unsigned long long *__restrict__ cost) {
    const uint32_t n = (uint32_t) *d_n;                  // U' (grid sized for the bound M)
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256u >= n) return;                  // (uniform)
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    const bool live = e < n;
    uint32_t g = 0xffffffffu;
    unsigned long long w = 0;
    if (live) {
        const uint4 t = tuples[idx_sorted[e]];
        ranges[e] = t;
        g = key_sorted[e];
        w = t.w;
    }
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t gl = __shfl(g, leader, PDL_WAVE);
        const bool in = live && g == gl;
        unsigned long long sum = in ? w : 0ull;
#pragma unroll
        for (int d = PDL_WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, PDL_WAVE);
        if ((int) lane == leader) atomicAdd(&cost[gl], sum);
        todo &= ~__ballot(in);
    }
}
// seq_off[s] = first range of gene s in the gene-sorted list (lower bound), seq_off[N] = number of ranges
// (the sorted field of a key is (key >> shift) & mask: the tuples of a multi-GPU build carry the owner rank above the gene)
__device__ __forceinline__ void seq_offset_of(uint32_t s, const uint32_t *__restrict__ key_sorted, const uint64_t *d_n, uint32_t n_seq,
                                              uint32_t *__restrict__ seq_off, uint32_t shift, uint32_t mask) {
    const uint32_t n = (uint32_t) *d_n;
    if (s > n_seq) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = lo + ((hi - lo) >> 1);
        if (((key_sorted[mid] >> shift) & mask) < s) lo = mid + 1; else hi = mid;
    }
    seq_off[s] = lo;
}
__global__ __launch_bounds__(256) void k_seq_offsets(const uint32_t *__restrict__ key_sorted, const uint64_t *d_n, uint32_t n_seq,
                                                     uint32_t *__restrict__ seq_off, uint32_t shift = 0, uint32_t mask = 0xffffffffu) {
    seq_offset_of(blockIdx.x * 256 + threadIdx.x, key_sorted, d_n, n_seq, seq_off, shift, mask);
}

// K-cost: per-genome cost (library.cpp:535-538); the total is their sum (library.cpp:337-349).
// Genes of a genome are usually adjacent, so a wave first tries to add up as one.  The three dataset-wide values
// (sum / max / min of kseq_lengths) are kept per lane over a grid-stride loop and leave the workgroup as ONE atomic each:
// same-address device atomics serialise at ~10-50 ns apiece, a wave's worth per 64 genes took longer than the sums.
struct GenomeCostArgs {
    const unsigned long long *cost; const uint32_t *kseq_len, *genome_of; uint32_t n_seq;
    unsigned long long *genome_cost, *sum_kseq, *max_kseq, *min_kseq;
};
__device__ __forceinline__ void genome_cost_by(const GenomeCostArgs &a, uint32_t block, uint32_t n_blocks) {
    const unsigned long long *__restrict__ cost = a.cost;
    const uint32_t *__restrict__ kseq_len = a.kseq_len, *__restrict__ genome_of = a.genome_of;
    const uint32_t n_seq = a.n_seq;
    unsigned long long *__restrict__ genome_cost = a.genome_cost, *__restrict__ sum_kseq = a.sum_kseq, *__restrict__ max_kseq = a.max_kseq, *__restrict__ min_kseq = a.min_kseq;
    __shared__ unsigned long long s_sum, s_max, s_min;
    if (threadIdx.x == 0) { s_sum = 0; s_max = 0; s_min = ~0ull; }
    pdl_sync();
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    unsigned long long ksum = 0, kmax = 0, kmin = ~0ull;
    for (uint32_t s0 = block * 256; s0 < n_seq; s0 += n_blocks * 256) {
        const uint32_t s = s0 + threadIdx.x;
        const bool live = s < n_seq;
        unsigned long long c = live ? cost[s] : 0ull;
        const unsigned long long kl = live ? (unsigned long long) kseq_len[s] : 0ull;
        const uint32_t g = live ? genome_of[s] : 0xffffffffu;
        ksum += kl; kmax = kl > kmax ? kl : kmax; if (kl && kl < kmin) kmin = kl;
        const uint32_t g0 = __shfl(g, 0, PDL_WAVE);
        if (__all(g == g0 || !live)) {
            unsigned long long csum = c;
#pragma unroll
            for (int d = PDL_WAVE / 2; d > 0; d >>= 1) csum += __shfl_down(csum, d, PDL_WAVE);
            if (lane == 0 && csum && g0 != 0xffffffffu) atomicAdd(&genome_cost[g0], csum);
        } else if (live && c) {
            atomicAdd(&genome_cost[g], c);
        }
    }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) {
        ksum += __shfl_down(ksum, d, PDL_WAVE);
        unsigned long long o = __shfl_down(kmax, d, PDL_WAVE);
        kmax = o > kmax ? o : kmax;
        o = __shfl_down(kmin, d, PDL_WAVE);
        kmin = o < kmin ? o : kmin;
    }
    if (lane == 0) { atomicAdd(&s_sum, ksum); atomicMax(&s_max, kmax); atomicMin(&s_min, kmin); }
    pdl_sync();
    if (threadIdx.x == 0 && s_sum) { atomicAdd(sum_kseq, s_sum); atomicMax(max_kseq, s_max); atomicMax(min_kseq, ~s_min); }   // min kept as a max of complements: zero-initialised like the rest
}
__global__ __launch_bounds__(256) void k_genome_cost(GenomeCostArgs a) { genome_cost_by(a, blockIdx.x, gridDim.x); }
// Option "fused_glue": the two kernels that close a build in ONE launch — the first `off_blocks` workgroups place the genes among
// the sorted ranges, the ones behind them add up the costs.  Neither half reads what the other writes.
__global__ __launch_bounds__(256) void k_close_build(const uint32_t *__restrict__ key_sorted, const uint64_t *d_n, uint32_t *__restrict__ seq_off, uint32_t gene_mask,
                                                     GenomeCostArgs a, uint32_t off_blocks) {
    if (blockIdx.x < off_blocks) seq_offset_of(blockIdx.x * 256 + threadIdx.x, key_sorted, d_n, a.n_seq, seq_off, 0u, gene_mask);
    else genome_cost_by(a, blockIdx.x - off_blocks, gridDim.x - off_blocks);
}

// K-cost: cost[] summed per genome into scalars[PDL_CTL_GCOST ..]; the k-mer statistics of the genes it adds up on the way
// go to scalars[w_sum] (sum), scalars[w_max] (max) and the word behind that (~min)
static GenomeCostArgs genome_cost_args(pdl_ctx *c, size_t w_sum, size_t w_max) {
    static_assert(PDL_CTL_KSEQ_NMIN == PDL_CTL_KSEQ_MAX + 1 && PDL_CTL_LAZY_KSEQ_MAX + 1 <= PDL_CTL_LAST, "~min sits behind max");
    unsigned long long *d_scal = c->scalars.as<unsigned long long>();
    return {c->cost.as<unsigned long long>(), c->kseq_len.as<uint32_t>(), c->d_gen, c->N, d_scal + PDL_CTL_GCOST, d_scal + w_sum, d_scal + w_max, d_scal + w_max + 1};
}
static uint32_t genome_cost_blocks(const pdl_ctx *c) { return std::min<uint32_t>((c->N + 255) / 256, 128); }
static void launch_genome_cost(pdl_ctx *c, size_t w_sum, size_t w_max) {
    hipLaunchKernelGGL(k_genome_cost, dim3(genome_cost_blocks(c)), dim3(256), 0, c->stream, genome_cost_args(c, w_sum, w_max));
    PDL_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Host side of the stages.  The words of the control block (c->scalars) are declared in pdl_common.h (PDL_CTL_*).
// ------------------------------------------------------------------------------------------------

// the rank table changes: c->rp, the letters, the key width — written here only (a build, an append, a removal)
static void adopt_rank_table(pdl_ctx *c, const RankParams &rp, const uint8_t present[256]) {
    c->rp = rp;
    memcpy(c->alpha_present, present, 256);
    c->key64 = rp.rank_bits > 32;
}

// K-hist + K-len + the rank table; leaves M, the rank parameters and the key width in the context.
static void stage_alphabet_and_lengths(pdl_ctx *c, int kvalue, bool only_complexity) {
    hipStream_t st = c->stream;
    if (kvalue <= 0) PDL_FAIL(PDL_ERR_KVALUE, "K value must be greater than 0.");
    // control block (PDL_CTL_*) — one allocation, one clearing fill, one device->host copy whenever the host looks
    // (device input whose genome ids are still on their way to the host: G is not known yet, at most N)
    const size_t ctl_words = PDL_CTL_GCOST + 2 * (size_t) (c->layout_deferred ? c->N : c->G);
    c->scalars.alloc(ctl_words * sizeof(uint64_t));
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    // K-len in one launch, which clears the control block itself (option "fused_glue" n > 1: up to min(n, KL_MAX_GENES) genes), or the
    // clearing launch here and the three-launch scan below
    const bool klen_one_launch = c->opt_fused_glue > 1 && c->N > 0 && ((uintptr_t) c->d_off & 15) == 0 && c->N <= std::min<uint32_t>((uint32_t) c->opt_fused_glue, KL_MAX_GENES);
    if (!klen_one_launch)
        hipLaunchKernelGGL(k_zero_u64, dim3((uint32_t) std::min<size_t>((ctl_words + 255) / 256, 1024)), dim3(256), 0, st, d_scal, ctl_words);     // (a kernel: a fill is a blit with ~10 us of barrier packets around it)

    ev_begin(c, EV_HIST);
    // K-len (independent of the histogram, reads the offsets only); its apply step also clears cost[], its total also lands in kmer_off[N]
    c->kseq_len.alloc((size_t) c->N * sizeof(uint32_t));
    c->gene_len.alloc((size_t) c->N * sizeof(uint32_t));
    c->kmer_off.alloc(((size_t) c->N + 1) * sizeof(uint64_t));
    c->cost.alloc((size_t) c->N * sizeof(uint64_t));
    if (klen_one_launch)
        hipLaunchKernelGGL(k_kseq_lengths, dim3((c->N + KL_TILE - 1) / KL_TILE), dim3(KL_THREADS), 0, st,
                           KlenArgs{c->d_off, c->R, (uint32_t) kvalue, c->N, c->kseq_len.as<uint32_t>(), c->gene_len.as<uint32_t>(), c->kmer_off.as<uint64_t>(),
                                    c->cost.as<unsigned long long>(), d_scal, (uint64_t) ctl_words});
    else
        scan_and_apply(c, c->N, KseqFlag{c->d_off, (uint32_t) kvalue},
                   KseqApply{c->kseq_len.as<uint32_t>(), c->gene_len.as<uint32_t>(), c->kmer_off.as<uint64_t>(), c->cost.as<unsigned long long>(), c->d_off, c->R,
                             reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_BAD_OFFSETS)}, d_scal + PDL_CTL_KMERS, c->kmer_off.as<uint64_t>() + c->N);
    if (c->layout_deferred) pdl_input_arrived(c);        // offsets[0] = 0 and offsets[N] = R checked before anything indexes residues
    if (c->R) {
        uint32_t blocks = (uint32_t) std::min<uint64_t>((c->R / 64 + HIST_THREADS - 1) / HIST_THREADS + 1, 2048);
        hipLaunchKernelGGL(k_hist, dim3(blocks), dim3(HIST_THREADS), 0, st, c->d_res, c->R,
                           reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_HIST));
    }
    uint64_t counters[256];
    uint64_t M = 0, bad = 0;
    {
        PinRead rd(c);
        const uint64_t *pc = rd.add<uint64_t>(d_scal, PDL_CTL_GCOST);          // scalars + histogram in one read
        ev_end(c, EV_HIST);
        rd.sync();
        memcpy(counters, pc + PDL_CTL_HIST, sizeof(counters));
        M = pc[PDL_CTL_KMERS]; bad = pc[PDL_CTL_BAD_OFFSETS];
    }
    if (bad) PDL_FAIL(PDL_ERR_ARGUMENT, "offsets must ascend from 0 to the residue count (%llu)", (unsigned long long) c->R);
    RankParams rp;
    uint8_t present[256];
    for (int i = 0; i < 256; i++) present[i] = counters[i] ? 1 : 0;
    rank_init_host(rp, counters, kvalue);
    adopt_rank_table(c, rp, present);
    c->M = M;
    c->only_complexity = only_complexity;
    if (M == 0) PDL_FAIL(PDL_ERR_EMPTY, "no gene is at least k=%d residues long: the dictionary is empty", kvalue);
    // the scan above sums in 32 bits: make sure it cannot have wrapped, and keep stream positions in u32
    if (c->R >= 0xfffffff0ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 residues (%llu) need 64-bit stream positions", (unsigned long long) c->R);
}

// K-rank over the whole stream into (keys_a, vals_a); d_bins != nullptr: also the interval histogram (multi-GPU build).
// Returns true when it has filed the counts of the rank sort's first pass in c->sort_tmp (pdl_sort_pairs, first_counts_filed).
template <class KeyT>
static bool stage_rank(pdl_ctx *c, uint32_t *d_bins = nullptr, uint32_t bin_shift = 0) {
    hipStream_t st = c->stream;
    const uint64_t M = c->M;
    c->keys_a.alloc(M * sizeof(KeyT)); c->keys_b.alloc(M * sizeof(KeyT));
    c->vals_a.alloc(M * sizeof(uint32_t)); c->vals_b.alloc(M * sizeof(uint32_t));
    if (c->rp.hash_fallback) {
        if constexpr (sizeof(KeyT) == 8) {
            if (d_bins) hipLaunchKernelGGL(k_rank_hash<1>, dim3((c->N + 255) / 256), dim3(256), 0, st, c->d_res, c->d_off,
                                           c->kmer_off.as<uint64_t>(), c->N, c->rp, c->keys_a.as<uint64_t>(), c->vals_a.as<uint32_t>(), d_bins);
            else hipLaunchKernelGGL(k_rank_hash<0>, dim3((c->N + 255) / 256), dim3(256), 0, st, c->d_res, c->d_off,
                                    c->kmer_off.as<uint64_t>(), c->N, c->rp, c->keys_a.as<uint64_t>(), c->vals_a.as<uint32_t>(), (uint32_t *) nullptr);
        }
    } else {
        const uint64_t tiles = (M + RANK_TILE - 1) / RANK_TILE;
        if (d_bins) hipLaunchKernelGGL((k_rank<KeyT, 1>), dim3((uint32_t) std::min<uint64_t>(tiles, 2048)), dim3(RANK_THREADS), 0, st, c->d_res, c->d_off,
                                       c->kmer_off.as<uint64_t>(), c->N, M, c->R, c->rp, c->keys_a.as<KeyT>(), c->vals_a.as<uint32_t>(), bin_shift, d_bins);
        else if (pdl_radix_lean(c, M)) {
            c->sort_tmp.alloc(pdl_radix_tmp_bytes(M));
            hipLaunchKernelGGL((k_rank<KeyT, 2>), dim3((uint32_t) ((M + PDL_RADIX_TILE - 1) / PDL_RADIX_TILE)), dim3(RANK_THREADS), 0, st, c->d_res, c->d_off,
                               c->kmer_off.as<uint64_t>(), c->N, M, c->R, c->rp, c->keys_a.as<KeyT>(), c->vals_a.as<uint32_t>(), 0u, c->sort_tmp.as<uint32_t>());
            PDL_HIP(hipGetLastError());
            return true;
        }
        else hipLaunchKernelGGL((k_rank<KeyT, 0>), dim3((uint32_t) tiles), dim3(RANK_THREADS), 0, st, c->d_res, c->d_off,
                                c->kmer_off.as<uint64_t>(), c->N, M, c->R, c->rp, c->keys_a.as<KeyT>(), c->vals_a.as<uint32_t>(), 0u, (uint32_t *) nullptr);
    }
    PDL_HIP(hipGetLastError());
    return false;
}

// K-rle of the sorted stream (keys, vals)[0 .. m): recpos, post and the record count at d_total.  Three launches (two for a
// short stream), as the generic scan it replaces under option "lean_records".
template <class KeyT>
static void rle_records(pdl_ctx *c, const KeyT *keys, const uint32_t *vals, uint64_t m, uint32_t *recpos, uint2 *post, uint64_t *d_total) {
    if (!c->opt_lean_records || c->opt_onepass_scan || m == 0) {
        scan_and_apply(c, m, RecHead<KeyT>{keys, vals}, RecScatter<KeyT>{keys, vals, m, recpos, post}, d_total);
        return;
    }
    const uint64_t tiles64 = (m + RLE_TILE - 1) / RLE_TILE;
    if (tiles64 > 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "scan of %llu elements exceeds the grid limit", (unsigned long long) m);
    const uint32_t tiles = (uint32_t) tiles64;
    c->scan_tmp.alloc((size_t) tiles * sizeof(uint32_t));
    uint32_t *ts = c->scan_tmp.as<uint32_t>();
    hipLaunchKernelGGL(k_rle_tile_sums<KeyT>, dim3(tiles), dim3(SCAN_THREADS), 0, c->stream, keys, vals, m, ts);
    if (tiles <= SCAN_INLINE_TILES) {
        hipLaunchKernelGGL((k_rle_apply<KeyT, true>), dim3(tiles), dim3(SCAN_THREADS), 0, c->stream, keys, vals, m, (const uint32_t *) ts, recpos, post, d_total, (uint64_t *) nullptr);
    } else {
        launch_tile_scan(c, ts, tiles, d_total, nullptr);
        hipLaunchKernelGGL((k_rle_apply<KeyT, false>), dim3(tiles), dim3(SCAN_THREADS), 0, c->stream, keys, vals, m, (const uint32_t *) ts, recpos, post, d_total, (uint64_t *) nullptr);
    }
    PDL_HIP(hipGetLastError());
}

// K-rle over the sorted stream (keys_b, vals_b)[0 .. m): records into c->post / recpos, their count into scalars[PDL_CTL_RECORDS].
template <class KeyT>
static void stage_dedup(pdl_ctx *c, uint64_t m) {
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    const KeyT *skeys = c->keys_b.as<KeyT>();
    const uint32_t *svals = c->vals_b.as<uint32_t>();
    ev_begin(c, EV_DICT);                                       // (ended by the caller, behind K-groups where it runs them)
    c->recpos.alloc((m + 1) * sizeof(uint32_t));
    c->post.alloc(m * sizeof(uint2));                           // U <= m records (sized before U is known)
    rle_records<KeyT>(c, skeys, svals, m, c->recpos.as<uint32_t>(), c->post.as<uint2>(), d_scal + PDL_CTL_RECORDS);
}

// K-sort + K-rle over the first m elements of (keys_in, vals_in): records into c->post / recpos.
// scalars[PDL_CTL_RECORDS] receives the record count.
template <class KeyT>
static void stage_sort_and_dedup(pdl_ctx *c, KeyT *keys_in, KeyT *keys_out, uint32_t *vals_in, uint32_t *vals_out, uint64_t m,
                                 bool first_counts_filed = false) {      // by K-rank, for all m elements (stage_rank)
    ev_begin(c, EV_SORT1);
    pdl_sort_pairs<KeyT>(c, keys_in, keys_out, vals_in, vals_out, m, c->rp.rank_bits, false, nullptr, 0, c->rp.key_bits == c->rp.rank_bits, first_counts_filed);
    ev_end(c, EV_SORT1);
    // remember which physical buffers hold the sorted stream (pdl_get_dictionary reads them)
    if ((void *) keys_out != c->keys_b.p) c->keys_a.swap(c->keys_b);
    if ((void *) vals_out != c->vals_b.p) c->vals_a.swap(c->vals_b);
    stage_dedup<KeyT>(c, m);
}

// The shard of a range build into ga: the genes that get range lists, as sorted gene-id intervals when every genome's genes
// are consecutive ids (the usual .faa) and there are at most GW_MAX_IV of them, and as the byte table.
static void group_shard_args(pdl_ctx *c, GroupTileArgs &ga) {
    hipStream_t st = c->stream;
    std::vector<uint2> &iv = c->h_own_iv;
    iv.clear();
    bool contiguous = true;
    for (uint32_t g : c->dict_shard) {               // (ascending genome ids; genomes in first-seen order: ascending gene ids too)
        const uint32_t b0 = c->h_genome_row_off[g], e0 = c->h_genome_row_off[g + 1];
        if (b0 == e0) continue;
        const uint32_t first = c->h_genome_rows[b0], last = c->h_genome_rows[e0 - 1];
        if (last - first + 1 != e0 - b0) { contiguous = false; break; }
        if (!iv.empty() && iv.back().y == first) iv.back().y = last + 1; else iv.push_back(make_uint2(first, last + 1));
    }
    if (contiguous) std::sort(iv.begin(), iv.end(), [](const uint2 &p, const uint2 &q) { return p.x < q.x; });
    for (size_t i = 1; contiguous && i < iv.size(); i++) if (iv[i].x < iv[i - 1].y) contiguous = false;      // (cannot happen: genes belong to one genome)
    if (contiguous && !iv.empty() && iv.size() <= GW_MAX_IV) {
        c->own_iv.alloc(iv.size() * sizeof(uint2));
        PDL_HIP(hipMemcpyAsync(c->own_iv.p, iv.data(), iv.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
        ga.own_iv = c->own_iv.as<uint2>(); ga.n_own_iv = (uint32_t) iv.size();
    }
    if (!c->dist) {                                  // (multi-GPU: the deal is on the device already, pdl_run_dist_finish)
        std::vector<uint8_t> &h = c->h_seq_in_shard; // lives in the context: the copy below needs no synchronisation
        h.assign((size_t) c->N, 0);
        std::vector<uint8_t> gsel((size_t) c->G, 0);
        for (uint32_t g : c->dict_shard) gsel[g] = 1;
        for (uint32_t i = 0; i < c->N; i++) h[i] = gsel[c->h_genome_of[i]];
        c->seq_in_shard.alloc(c->N);
        PDL_HIP(hipMemcpyAsync(c->seq_in_shard.p, h.data(), c->N, hipMemcpyHostToDevice, st));
    }
    ga.in_shard = c->seq_in_shard.as<uint8_t>();
}

// ---- the range stage: K-groups + K-ranges + K-cost -------------------------------------------------------------------------------
// What the five paths that build range lists share ("The host side of the range stage"): the whole build and the append / remove tail
// (stage_ranges_and_costs), the next genome batch (pdl_run_reshard), the multi-GPU owner (pdl_run_dist_finish) and sender (pdl_run_dist_ranges, _finish_ranges).
// mode 0: whole groups for the shard's genes | 1: upper ranges, every gene | 2: upper ranges, the shard's genes.

// What a path clears of the control block, by name: an inclusive span of PDL_CTL_* words, the per-genome words, cost[].
static void clear_ctl(pdl_ctx *c, size_t first, size_t last) { PDL_HIP(hipMemsetAsync(c->scalars.as<uint64_t>() + first, 0, (last - first + 1) * sizeof(uint64_t), c->stream)); }
static void clear_genome_words(pdl_ctx *c, bool upper_too = true) {      // [G] costs (+ [G] lookups above the diagonal)
    PDL_HIP(hipMemsetAsync(c->scalars.as<uint64_t>() + PDL_CTL_GCOST, 0, (upper_too ? 2 : 1) * (size_t) c->G * sizeof(uint64_t), c->stream));
}
static void clear_kseq_stats(pdl_ctx *c) { clear_ctl(c, PDL_CTL_KSEQ_SUM, PDL_CTL_KSEQ_SUM); clear_ctl(c, PDL_CTL_KSEQ_MAX, PDL_CTL_KSEQ_NMIN); }   // k_genome_cost's sum | max, ~min
static void clear_gene_costs(pdl_ctx *c) { PDL_HIP(hipMemsetAsync(c->cost.p, 0, (size_t) c->N * sizeof(uint64_t), c->stream)); }

// How a path's ranges travel and what their buffers are sized for.
//   packed    8 bytes, carried through the gene sort as its payload (no gather afterwards): whenever a range sits right behind its
//             own record (the upper modes) and a posting count fits 22 bits; else 16-byte tuples fetched through the sorted positions
//   exact     the COUNT pass's total is read (one synchronisation) and the buffers are sized for it: a shard (modes 0, 2: 1/W or one
//             batch of the genes) and a rank's run — a 512-genome set would otherwise allocate 20-28 bytes for each of its 0.9 G
//             records per shard.  Else (the whole build on one GPU, mode 1) the host does not look: the range count stays on the
//             device, buffers and kernels are sized for the bound (every record may get a range)
//   fused     single-GPU build with packed ranges: the tuples are filed by the low byte of their gene by the kernel that makes
//             them (the first pass of the gene sort without a trip through HBM in between)
//   received  the gene sort's first pair is the caller's inbox (pdl_run_dist_finish_ranges): only the second is carved
struct RangePlan { bool packed, exact, fused, received; };
static RangePlan range_plan(const pdl_ctx *c, int mode, bool run_of_a_rank = false) {
    const bool packed = mode != 0 && c->N < (1u << 22);
    return RangePlan{packed, mode != 1 || run_of_a_rank, mode == 1 && packed && !run_of_a_rank, false};
}
constexpr RangePlan RANGES_RECEIVED{true, true, false, true};

// c->scratch for `cap` ranges:
//   packed    pay_a u64[cap] | pay_b u64[cap] | [k2a u32[cap]] | k2b u32[cap]
//   tuples    tuples uint4[cap] | v2a u32[cap] | [k2a u32[cap]] | k2b u32[cap] | v2b u32[cap]
//   received  pay_b u64[cap] | k2b u32[cap]          (the outbox in `scratch` has been delivered: its memory takes this pair)
// k2a, the gene sort's first key buffer: in `scratch` when exact (the rank sort's buffers may be gone: "low_memory"), else vals_a (free after sort 1)
struct RangeBufs { uint4 *tuples; unsigned long long *pay_a, *pay_b; uint32_t *k2a, *k2b, *v2a, *v2b; };
static RangeBufs carve_ranges(pdl_ctx *c, const RangePlan &p, uint64_t cap, uint32_t *in_keys = nullptr, unsigned long long *in_ranges = nullptr) {
    const size_t first = p.received ? 0 : p.packed ? sizeof(uint64_t) : sizeof(uint4) + sizeof(uint32_t);      // pay_a, or tuples and v2a
    const size_t second = p.packed ? sizeof(uint64_t) + sizeof(uint32_t) : 2 * sizeof(uint32_t);              // pay_b and k2b, or k2b and v2b
    const bool k2a_here = p.exact && !p.received;
    c->scratch.alloc(cap * (first + second + (k2a_here ? sizeof(uint32_t) : 0)) + 64);
    RangeBufs b{};
    if (p.packed) {
        b.pay_a = p.received ? in_ranges : c->scratch.as<unsigned long long>();
        b.pay_b = p.received ? c->scratch.as<unsigned long long>() : b.pay_a + cap;
        b.k2b = reinterpret_cast<uint32_t *>(b.pay_b + cap);
    } else {
        b.tuples = c->scratch.as<uint4>();
        b.v2a = reinterpret_cast<uint32_t *>(b.tuples + cap); b.k2b = b.v2a + cap;
    }
    if (p.received) b.k2a = in_keys;
    else if (k2a_here) { b.k2a = b.k2b; b.k2b += cap; }
    else { c->vals_a.alloc(cap * sizeof(uint32_t)); b.k2a = c->vals_a.as<uint32_t>(); }
    if (!p.packed) b.v2b = b.k2b + cap;
    return b;
}

// Where a WRITE pass writes: the ranges into b (k_group_write; k_range_scatter is told its own), and its copy of the postings'
// head bits, one bit per record: for the per-gene costs made on demand (packed ranges).
static void set_write_targets(pdl_ctx *c, GroupTileArgs &ga, const RangeBufs &b) {
    c->head_bits.alloc(((ga.n_bound + GW_TILE - 1) / GW_TILE) * GW_ROUNDS * sizeof(uint64_t));
    ga.head_bits = c->head_bits.as<unsigned long long>();
    ga.key2 = b.k2a; ga.tuples = b.tuples; ga.pay8 = b.pay_a;
}

// An exact plan's two passes: COUNT, the range count read (with `tasks_meanwhile`, the task layout is made while the device
// counts: host work + small uploads), buffers for max(count, 1) ranges into b, WRITE.  Returns the count.
static uint64_t count_then_write(pdl_ctx *c, GroupTileArgs &ga, uint32_t grid, int mode, const RangePlan &plan, bool tasks_meanwhile, RangeBufs &b) {
    launch_range_count(c, ga, grid, mode);
    if (tasks_meanwhile && !c->tasks_ready) pdl_prepare_tasks(c);
    PinRead rd(c);
    const uint64_t *pn = rd.add<uint64_t>(c->scalars.as<uint64_t>() + PDL_CTL_RANGES, 1);
    rd.sync();
    const uint64_t n = pn[0];
    b = carve_ranges(c, plan, std::max<uint64_t>(n, 1));
    set_write_targets(c, ga, b);
    launch_range_write(c, ga, grid, mode);
    return n;
}

// K-seq-offsets: every gene's place among the ranges sorted by gene (the gene of a key: its bits under gene_mask)
// with_cost (a build's own range stage under option "fused_glue"): K-cost, which would be the next launch, rides in this one
static void launch_seq_offsets(pdl_ctx *c, const uint32_t *keys_by_gene, uint32_t gene_mask, bool with_cost = false) {
    c->seq_off.alloc(((size_t) c->N + 1) * sizeof(uint32_t));
    const uint32_t off_blocks = (c->N + 1 + 255) / 256;
    const uint64_t *d_n = c->scalars.as<uint64_t>() + PDL_CTL_RANGES;
    if (with_cost)
        hipLaunchKernelGGL(k_close_build, dim3(off_blocks + genome_cost_blocks(c)), dim3(256), 0, c->stream, keys_by_gene, d_n, c->seq_off.as<uint32_t>(), gene_mask,
                           genome_cost_args(c, PDL_CTL_KSEQ_SUM, PDL_CTL_KSEQ_MAX), off_blocks);
    else hipLaunchKernelGGL(k_seq_offsets, dim3(off_blocks), dim3(256), 0, c->stream, keys_by_gene, d_n, c->N, c->seq_off.as<uint32_t>(), 0u, gene_mask);
    PDL_HIP(hipGetLastError());
}
static uint32_t gene_id_bits(const pdl_ctx *c) { return std::max<uint32_t>(1, bit_length64(c->N ? c->N - 1 : 0)); }

// Packed ranges, by gene: the sort of n_sort pairs (their count at d_sort_n, or n_sort itself; none: no sort) over the gene bits from first_bit on into
// (k2b, pay_b), the genes' offsets, and the context's view: the join reads the ranges where the sort left them.  Ends EV_SORT2 (the caller's), spans EV_RANGES.
static void sort_ranges_by_gene(pdl_ctx *c, RangeBufs b, uint64_t n_sort, const uint64_t *d_sort_n, uint32_t first_bit, uint32_t gene_mask, bool with_cost = false) {
    if (n_sort) pdl_sort_pairs<uint32_t, unsigned long long>(c, b.k2a, b.k2b, b.pay_a, b.pay_b, n_sort, gene_id_bits(c), false, d_sort_n, first_bit, true);
    ev_end(c, EV_SORT2); ev_begin(c, EV_RANGES);
    c->ranges8 = reinterpret_cast<const uint2 *>(b.pay_b); c->upper_only = true;
    launch_seq_offsets(c, b.k2b, gene_mask, with_cost);
    ev_end(c, EV_RANGES);
}

// K-ranges of stage_ranges_and_costs: the range lists of `mode` from the postings of ga, gene major, by the plan.  with_cost: K-cost
// rides in the last launch (launch_seq_offsets).
static void build_ranges(pdl_ctx *c, GroupTileArgs &ga, uint32_t grid, int mode, bool with_cost) {
    hipStream_t st = c->stream;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    const uint64_t bound = ga.n_bound, *d_us = d_scal + PDL_CTL_RANGES;       // d_us: ranges built = the total of the tile counts
    const RangePlan plan = range_plan(c, mode);
    ev_begin(c, EV_SORT2);
    if (mode != 1) group_shard_args(c, ga);                // only the genes this context scores need range lists
    RangeBufs b{};
    uint64_t n_sort = bound;                               // what the kernels behind the passes are sized for: the bound, the count at d_sort_n ...
    const uint64_t *d_sort_n = d_us;
    uint32_t first_bit = 0;                                // (fused: the gene sort's first digit is done)
    if (plan.exact) {                                      // ... or the count the host has read
        n_sort = std::max<uint64_t>(count_then_write(c, ga, grid, mode, plan, true, b), 1); d_sort_n = nullptr;
    } else {
        b = carve_ranges(c, plan, bound);
        set_write_targets(c, ga, b);
        if (plan.fused) {
            const uint32_t n_tiles4 = (uint32_t) ((bound + PDL_RADIX_TILE - 1) / PDL_RADIX_TILE);
            const size_t table = (size_t) PDL_RADIX_BINS * n_tiles4, tiles = (bound + GW_TILE - 1) / GW_TILE;
            // (the scan below uses scan_tmp: the per-tile heads move next to the radix tables)
            c->sort_tmp.alloc((2 * table + PDL_RADIX_BINS + 3 * tiles + 1) * sizeof(uint32_t));
            uint32_t *counts = c->sort_tmp.as<uint32_t>(), *offs = counts + table, *digit_total = offs + table;
            ga.tile_sums = digit_total + PDL_RADIX_BINS; ga.th_first = ga.tile_sums + tiles; ga.th_last = ga.th_first + tiles; ga.chunk_sums = nullptr;
            const uint32_t grid4 = std::max<uint32_t>(1, std::min<uint32_t>(n_tiles4, (uint32_t) c->cus * 8));
            if (c->opt_lean_records) hipLaunchKernelGGL(k_range_count_hist<true>, dim3(grid4), dim3(GW_THREADS), 0, st, ga, n_tiles4, counts);
            else hipLaunchKernelGGL(k_range_count_hist<false>, dim3(grid4), dim3(GW_THREADS), 0, st, ga, n_tiles4, counts);
            const uint32_t *totals = pdl_radix_offsets(c, counts, offs, n_tiles4, d_scal + PDL_CTL_RANGES, digit_total);
            hipLaunchKernelGGL(k_range_scatter, dim3(n_tiles4), dim3(GW_THREADS), 0, st, ga, n_tiles4, offs, b.k2b, b.pay_b, totals, d_scal + PDL_CTL_RANGES);
            PDL_HIP(hipGetLastError());
            // pass 1 of the gene sort is done: (k2b, pay_b) hold its output, the remaining passes go on from there
            std::swap(b.k2a, b.k2b); std::swap(b.pay_a, b.pay_b); first_bit = 8;
        } else {
            launch_range_count(c, ga, grid, mode);
            launch_range_write(c, ga, grid, mode);
        }
    }
    if (plan.packed) {
        sort_ranges_by_gene(c, b, n_sort, d_sort_n, first_bit, 0xffffffffu, with_cost);
    } else {                                               // values = tuple positions: sorted pairs in (k2b, v2b), the tuples fetched through them
        pdl_sort_pairs<uint32_t>(c, b.k2a, b.k2b, b.v2a, b.v2b, n_sort, gene_id_bits(c), true, d_sort_n, 0, true);
        ev_end(c, EV_SORT2); ev_begin(c, EV_RANGES);
        c->ranges8 = nullptr; c->upper_only = mode != 0;
        c->ranges.alloc(std::max<uint64_t>(n_sort, 1) * sizeof(uint4));
        const uint32_t gblocks = (uint32_t) std::max<uint64_t>((n_sort + 255) / 256, 1);
        hipLaunchKernelGGL(k_gather_ranges, dim3(gblocks), dim3(256), 0, st, b.v2b, b.k2b, b.tuples, d_us, c->ranges.as<uint4>(), c->cost.as<unsigned long long>());
        launch_seq_offsets(c, b.k2b, 0xffffffffu, with_cost);
        ev_end(c, EV_RANGES);
    }
}

// The closing read of a build: `words` of the control block from word 0 on and the look-back error word, which is checked.  Decodes
// the k-mer statistics k_genome_cost added up: sum, max, and the min kept as a max of complements (still zero: no gene has a k-mer).
static const uint64_t *closing_read(pdl_ctx *c, PinRead &rd, size_t words) {
    const uint64_t *pt = rd.add<uint64_t>(c->scalars.as<uint64_t>(), words);
    const uint32_t *lbe = lookback_error_word(c, rd);
    rd.sync();
    lookback_check(c, lbe);
    c->sum_kseq = pt[PDL_CTL_KSEQ_SUM]; c->max_kseq = pt[PDL_CTL_KSEQ_MAX]; c->min_kseq = pt[PDL_CTL_KSEQ_NMIN] == 0 ? 1 : ~pt[PDL_CTL_KSEQ_NMIN];
    return pt;
}

// Waits for the stream and closes the range stage's timings; returns the time of `total_event`, which spans the call.
static float close_range_timings(pdl_ctx *c, int total_event) {
    PDL_HIP(hipStreamSynchronize(c->stream));
    c->tm.sort_seq_ms = ev_ms(c, EV_SORT2); c->tm.ranges_ms = ev_ms(c, EV_RANGES);
    return ev_ms(c, total_event);
}

// K-groups + K-ranges + K-cost over the dictionary (postings with head bits; `bound` records at most, the count is at
// scalars[PDL_CTL_RECORDS]): fold the last record; complexity-only costs, or the ranges of `mode`; genome costs; closing read.
static void stage_ranges_and_costs(pdl_ctx *c, uint64_t bound, int mode, bool only_complexity) {
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    GroupPlan gp = group_tiles_plan(c, pdl_postings(c), bound, d_scal + PDL_CTL_RECORDS);
    gp.a.cost = c->cost.as<unsigned long long>();
    gp.a.counters = reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_COUNTERS);
    hipLaunchKernelGGL(k_fold_last_record, dim3(1), dim3(1024), 0, c->stream, gp.a.post, c->post_ext ? (uint32_t *) nullptr : c->recpos.as<uint32_t>(), gp.a.d_n);
    const bool cost_rides = c->opt_fused_glue && !only_complexity && c->N > 0;     // K-cost in K-seq-offsets' launch
    if (only_complexity) { c->ranges8 = nullptr; launch_group_costs<false, true>(c, gp.a, gp.grid); }    // (cost[] was zeroed by K-len's apply, the counters with the control block)
    else build_ranges(c, gp.a, gp.grid, mode, cost_rides);
    // packed ranges: "Total cost" straight from the WRITE pass; per-gene / per-genome costs on demand (pdl_ensure_costs)
    c->costs_ready = c->ranges8 == nullptr;
    if (!cost_rides) launch_genome_cost(c, PDL_CTL_KSEQ_SUM, PDL_CTL_KSEQ_MAX);       // K-cost
    PinRead rd(c);                           // one copy: the whole control block
    const uint64_t *pt = closing_read(c, rd, PDL_CTL_GCOST + (size_t) c->G);
    c->h_genome_cost.assign(pt + PDL_CTL_GCOST, pt + PDL_CTL_GCOST + c->G);     // (a shard, one rank of several: its own genomes only)
    c->U = pt[PDL_CTL_RECORDS]; c->Ushared = pt[PDL_CTL_SHARED]; c->Urepeat = pt[PDL_CTL_REPEATS]; c->NG = pt[PDL_CTL_GROUPS];
    c->P = c->costs_ready ? 0 : pt[PDL_CTL_OWN_COST];
    if (c->costs_ready) for (uint64_t v : c->h_genome_cost) c->P += v;
}

// ---- the ranges again, for another shard of genomes, on the dictionary that is there ---------------------------------------------
// (scoring a large set a batch of genomes at a time: the postings — rank, sort, dedup, most of the build — are made once; a batch
// costs the two passes over the postings that form its genes' range lists.)  The postings are as the first build left them,
// group-head bits included (a WRITE pass only reads them); the counters of the range stage start at zero again.
void pdl_run_reshard(pdl_ctx *c) {
    if (c->dist || c->post_ext) PDL_FAIL(PDL_ERR_STATE, "genome shard: a multi-GPU context deals the genomes itself");
    if (c->dict_shard.empty() || c->upper_only) PDL_FAIL(PDL_ERR_STATE, "genome shard: the dictionary was built for all genomes; set the first shard before pdl_preprocess");
    ev_begin(c, EV_PRE_TOTAL);
    clear_ctl(c, PDL_CTL_RANGES, PDL_CTL_RANGES);
    clear_ctl(c, PDL_CTL_COUNTERS, PDL_CTL_LAST);
    clear_genome_words(c);
    clear_gene_costs(c);
    // (k_genome_cost adds the k-mer statistics of all genes up once more: they are taken from the first build)
    const uint64_t sum_kseq = c->sum_kseq, max_kseq = c->max_kseq, min_kseq = c->min_kseq;
    clear_kseq_stats(c);
    c->dict_shard = c->shard;
    c->tasks_ready = false;
    ev_begin(c, EV_DICT); ev_end(c, EV_DICT);
    stage_ranges_and_costs(c, c->U, 0, false);
    c->sum_kseq = sum_kseq; c->max_kseq = max_kseq; c->min_kseq = min_kseq;
    ev_end(c, EV_PRE_TOTAL);
    c->tm.reshard_ms = close_range_timings(c, EV_PRE_TOTAL);
}

// cost[] (per gene) and h_genome_cost (per genome), when the build left them for later (packed ranges)
void pdl_ensure_costs(pdl_ctx *c) {
    if (c->costs_ready) return;
    hipStream_t st = c->stream;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    clear_gene_costs(c);
    clear_genome_words(c, false);
    const uint32_t n = (uint32_t) c->U;
    hipLaunchKernelGGL(k_gene_costs_lazy, dim3((n + 255) / 256), dim3(256), 0, st, pdl_postings(c), c->head_bits.as<unsigned long long>(), n,
                       c->cost.as<unsigned long long>());
    // per genome (the kseq statistics it also adds up go to scratch words)
    launch_genome_cost(c, PDL_CTL_LAZY_KSEQ_SUM, PDL_CTL_LAZY_KSEQ_MAX);
    PinRead rd(c);
    const uint64_t *pg = rd.add<uint64_t>(d_scal + PDL_CTL_GCOST, c->G);
    rd.sync();
    c->h_genome_cost.assign(pg, pg + c->G);
    c->costs_ready = true;
}

// option low_memory, behind a build (the stream has been waited for): what only the build needed goes back — the sorted k-mer
// stream with it, so pdl_get_dictionary and the incremental entry points are not available then.  Packed ranges live in
// `scratch`: it stays.
static void release_build_buffers(pdl_ctx *c) {
    c->keys_a.release(); c->keys_b.release(); c->vals_a.release(); c->vals_b.release(); c->recpos.release(); c->sort_tmp.release();
}

template <class KeyT>
static void dictionary_pipeline(pdl_ctx *c, bool only_complexity) {
    const uint64_t M = c->M;
    ev_begin(c, EV_RANK);
    const bool counts_filed = stage_rank<KeyT>(c);
    ev_end(c, EV_RANK);
    KeyT *keys_in = c->keys_a.as<KeyT>(), *keys_out = c->keys_b.as<KeyT>();
    uint32_t *vals_in = c->vals_a.as<uint32_t>(), *vals_out = c->vals_b.as<uint32_t>();
    stage_sort_and_dedup<KeyT>(c, keys_in, keys_out, vals_in, vals_out, M, counts_filed);
    ev_end(c, EV_DICT);
    if (c->layout_deferred) pdl_finish_layout(c);   // device input: the genome layout is host work too, and nothing before this point needed it
    if (c->opt_alphabet_rekey) {                    // (G is known from here on; the residues are still the caller's to read)
        c->rk.short_letters.alloc((size_t) c->G * 32);
        hipLaunchKernelGGL(k_zero_u64, dim3((uint32_t) std::min<size_t>(((size_t) c->G * 4 + 255) / 256, 1024)), dim3(256), 0, c->stream,
                           c->rk.short_letters.as<uint64_t>(), (size_t) c->G * 4);
        hipLaunchKernelGGL(k_short_letters, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->d_res, c->d_off, c->d_gen, c->N, c->G, c->rp.k, c->R,
                           c->rk.short_letters.as<uint32_t>());
        PDL_HIP(hipGetLastError());
    }
    if (!only_complexity) pdl_prepare_tasks(c);     // host work + small uploads while the device sorts
    // U (records) and the range count stay on the device until the end of the build: everything below is sized and
    // launched for the bound M and reads the counts there — no host round trip in the middle of the pipeline
    stage_ranges_and_costs(c, M, c->dict_shard.empty() ? 1 : 0, only_complexity);
    if (c->opt_low_memory) {
        PDL_HIP(hipStreamSynchronize(c->stream));
        release_build_buffers(c);
    }
}

// ------------------------------------------------------------------------------------------------
// What the incremental rebuilds (K-append, K-remove) share.  Both read the context only until the host has decided about the
// alphabet (rk_change, pdl_rekey.h), commit (commit_set_change), leave a sorted stream of the new set in (keys_b, vals_b) and then
// run the build's own stages on it (rebuild_behind_sort); the next entry point that changes the set does the same through these.
// ------------------------------------------------------------------------------------------------
// The commit of a call that changes the set, behind its last refusal: the context changes, and where the letters do (ch.rekey) it
// takes the new rank table.  Returns what the tail needs: the width of the keys that are there, and the call's pdl_rekey_info
// but for its time; `keys_rewritten` is the stream K-rekey will go over.
struct SetCommit { bool key64_before; pdl_rekey_info ri; };
static SetCommit commit_set_change(pdl_ctx *c, const RkChange &ch, uint64_t keys_rewritten) {
    pdl_stale(c, Stale::build);         // "from here on the context changes": what was derived from the old set is stale, and a failure leaves the context un-preprocessed
    SetCommit sc{c->key64, pdl_rekey_info{}};
    pdl_rekey_info &ri = sc.ri;
    ri.letters_before = ri.letters_after = c->rp.base; ri.key_bits_before = ri.key_bits_after = c->rp.rank_bits;
    if (ch.rekey) {
        adopt_rank_table(c, ch.rp, ch.present);
        ri.letters_after = ch.rp.base; ri.key_bits_after = ch.rp.rank_bits; ri.keys_rewritten = keys_rewritten; ri.rekeyed = 1;
    }
    return sc;
}

// Where the genome ids are on the device: c->d_gen is the context's own buffer (Own: an append grows it in place), an ingest
// buffer of the context's, or a caller's — which may be gone: the host copy (h_genome_of) serves then.
enum class GenomeIds { Callers, Ingest, Own };
static GenomeIds genome_ids_on_device(const pdl_ctx *c) {
    if (!c->d_gen) return GenomeIds::Callers;
    return c->d_gen == c->own_gen.p ? GenomeIds::Own : c->d_gen == c->in_gen.p || c->d_gen == c->ing_gen.p ? GenomeIds::Ingest : GenomeIds::Callers;
}

// The tail behind the sort, for a set of N1 genes in G1 genomes (the layout of the host is the new one already) whose k-mers
// are M1 sorted entries: control block and costs cleared for the new sizes, then — behind `queue_stream`, which queues
// whatever still has to bring the stream into (keys_b, vals_b), K-rekey (rekey_in_place) included — K-rle, the task layout,
// K-groups / K-ranges / K-cost.  The device work is the second stretch of c->set_spans; the stream has been waited for on return,
// low_memory has taken its buffers and K-rekey's old keys are gone.  Closes the call's books: c->last_rekey is `ri` with its time;
// c->tm starts from zero (the scoring fields start again) with the tail's fields and the total, the caller adds rank_ms and
// sort_rank_ms from the stage events, which are unused here unless queue_stream used them.
template <class QueueStream>
static void rebuild_behind_sort(pdl_ctx *c, pdl_rekey_info ri, uint64_t M1, uint32_t N1, uint32_t G1, QueueStream &&queue_stream) {
    hipStream_t st = c->stream;
    EventSpans<2> &spans = c->set_spans;
    const size_t ctl_words = PDL_CTL_GCOST + 2 * (size_t) G1;
    c->scalars.alloc(ctl_words * sizeof(uint64_t));
    c->cost.alloc((size_t) N1 * sizeof(uint64_t));
    c->ev[EV_HIST].used = c->ev[EV_RANK].used = c->ev[EV_SORT1].used = c->ev[EV_MERGE].used = c->ev[EV_REKEY].used = false;
    spans.begin();
    hipLaunchKernelGGL(k_zero_u64, dim3((uint32_t) std::min<size_t>((ctl_words + 255) / 256, 1024)), dim3(256), 0, st, c->scalars.as<uint64_t>(), ctl_words);
    hipLaunchKernelGGL(k_zero_u64, dim3((uint32_t) std::min<size_t>(((size_t) N1 + 255) / 256, 1024)), dim3(256), 0, st, c->cost.as<uint64_t>(), (size_t) N1);
    PDL_HIP(hipGetLastError());
    queue_stream();
    pdl_with_key(c->key64, [&](auto key) { stage_dedup<decltype(key)>(c, M1); });
    ev_end(c, EV_DICT);
    pdl_prepare_tasks(c);
    stage_ranges_and_costs(c, M1, 1, false);
    spans.end();
    PDL_HIP(hipStreamSynchronize(st));
    if (c->opt_low_memory) release_build_buffers(c);
    c->rk.keys.release();
    ri.rekey_ms = ev_ms(c, EV_REKEY);
    c->last_rekey = ri;
    pdl_timings t{};
    t.dict_ms = ev_ms(c, EV_DICT); t.sort_seq_ms = ev_ms(c, EV_SORT2); t.ranges_ms = ev_ms(c, EV_RANGES);
    t.preprocess_total_ms = spans.ms(0) + spans.ms(1);
    c->tm = t;
}

// K-rank of genes that are not the context's input (a query, an append) with the rank parameters `rp` — the context's, or the
// union's of a query that brings letters: gene values 0..n-1
template <class KeyT>
static void rank_new_genes(pdl_ctx *c, const RankParams &rp, const uint8_t *res, const uint64_t *off, const uint64_t *kmer_off, uint32_t n, uint64_t m,
                           uint64_t n_res, KeyT *keys, uint32_t *vals) {
    hipStream_t st = c->stream;
    if (rp.hash_fallback) {
        if constexpr (sizeof(KeyT) == 8)
            hipLaunchKernelGGL(k_rank_hash<0>, dim3((n + 255) / 256), dim3(256), 0, st, res, off, kmer_off, n, rp, keys, vals, (uint32_t *) nullptr);
    } else {
        const uint64_t tiles = (m + RANK_TILE - 1) / RANK_TILE;
        hipLaunchKernelGGL((k_rank<KeyT, 0>), dim3((uint32_t) tiles), dim3(RANK_THREADS), 0, st, res, off, kmer_off, n, m, n_res, rp,
                           keys, vals, 0u, (uint32_t *) nullptr);
    }
    PDL_HIP(hipGetLastError());
}

const void *pdl_query_dictionary(pdl_ctx *c, const RankParams &rp, bool key64, const uint8_t *res, const uint64_t *off, const uint64_t *kmer_off,
                                 uint32_t n, uint64_t m, uint64_t n_res, void *keys_a, void *keys_b, uint32_t *vals_a, uint32_t *vals_b,
                                 uint32_t *recpos, uint2 *post, uint64_t *d_u) {
    return pdl_with_key(key64, [&](auto key) -> const void * {
        using KeyT = decltype(key);
        KeyT *keys_in = static_cast<KeyT *>(keys_a), *keys_out = static_cast<KeyT *>(keys_b);
        rank_new_genes<KeyT>(c, rp, res, off, kmer_off, n, m, n_res, keys_in, vals_a);
        pdl_sort_pairs<KeyT>(c, keys_in, keys_out, vals_a, vals_b, m, rp.rank_bits, false, nullptr, 0, rp.key_bits == rp.rank_bits);
        rle_records<KeyT>(c, keys_out, vals_b, m, recpos, post, d_u);
        return keys_out;
    });
}
const void *pdl_query_dictionary(pdl_ctx *c, const uint8_t *res, const uint64_t *off, const uint64_t *kmer_off, uint32_t n, uint64_t m,
                                 uint64_t n_res, void *keys_a, void *keys_b, uint32_t *vals_a, uint32_t *vals_b, uint32_t *recpos, uint2 *post,
                                 uint64_t *d_u) {
    return pdl_query_dictionary(c, c->rp, c->key64, res, off, kmer_off, n, m, n_res, keys_a, keys_b, vals_a, vals_b, recpos, post, d_u);
}

// ---- option "query_rekey": the host's alphabet decision for a query or a chunk of queries, and what it queues (pdl_rekey.h) ------
bool pdl_query_rekey_base_exact(const pdl_ctx *c, const char **why) {
    if (rk_exact(c->rp)) return true;
    *why = rk_why_not(c->rp);
    return false;
}
bool pdl_query_rekey_plan(pdl_ctx *c, const uint32_t letters[8], bool adopt, const char **why) {
    RkQuery q;
    if (!rk_query(c->rp, c->alpha_present, letters, q)) { *why = rk_why_not(q.up.rp); return false; }
    if (!adopt) return true;
    auto &rk = c->qb.rk;
    hipStream_t st = c->stream;
    rk.rp = q.up.rp; rk.key64 = q.up.rp.rank_bits > 32;
    rk.up = q.up.args; rk.down = q.down;
    memcpy(rk.absent, q.absent, sizeof(rk.absent));
    rk.h_up.swap(q.up_table); rk.h_down.swap(q.down_table);
    rk.up_table.alloc(rk.h_up.size() * 8);
    PDL_HIP(hipMemcpyAsync(rk.up_table.p, rk.h_up.data(), rk.h_up.size() * 8, hipMemcpyHostToDevice, st));
    const void *h_down = rk.h_down.data();
    const size_t kb = c->key64 ? 8 : 4;
    if (!c->key64) {                                                        // (B^k <= 2^32: every entry fits)
        rk.h_down32.assign(rk.h_down.begin(), rk.h_down.end());
        h_down = rk.h_down32.data();
    }
    rk.down_table.alloc(rk.h_down.size() * kb);
    PDL_HIP(hipMemcpyAsync(rk.down_table.p, h_down, rk.h_down.size() * kb, hipMemcpyHostToDevice, st));
    return true;
}
void pdl_query_rebase(pdl_ctx *c, const void *qkeys, const uint32_t *recpos, const unsigned long long *d_records, uint64_t bound) {
    auto &rk = c->qb.rk;
    hipStream_t st = c->stream;
    const size_t kb = c->key64 ? 8 : 4;
    rk.up3.alloc(3 * 8); rk.bkey.alloc(std::max<uint64_t>(bound, 1) * kb); rk.none.alloc(std::max<uint64_t>(bound, 1));
    RkAbsent ab;
    memcpy(ab.bits, rk.absent, sizeof(ab.bits));
    const bool timed = c->opt_stage_timers;
    rk.span.start(st);
    pdl_with_keys_up(c->key64, rk.key64, [&](auto key_b, auto key_q) {
        using KeyB = decltype(key_b);
        using KeyQ = decltype(key_q);
        hipLaunchKernelGGL(k_q_up3<KeyB>, dim3(1), dim3(64), 0, st, (const KeyB *) c->keys_b.as<KeyB>(), (const uint32_t *) c->recpos.as<uint32_t>(),
                           (uint32_t) c->U, c->M, rk.up, (const uint64_t *) rk.up_table.as<uint64_t>(), rk.up3.as<unsigned long long>());
        if (!bound) return;
        if (timed) rk.span.begin();
        hipLaunchKernelGGL((k_q_rebase<KeyQ, KeyB>), dim3((uint32_t) ((bound + RK_THREADS - 1) / RK_THREADS)), dim3(RK_THREADS),
                           (size_t) rk.down.entries * sizeof(KeyB), st, static_cast<const KeyQ *>(qkeys), recpos, d_records, bound, rk.down,
                           (const KeyB *) rk.down_table.as<KeyB>(), ab, rk.bkey.as<KeyB>(), rk.none.as<uint8_t>());
        if (timed) rk.span.end();
    });
    PDL_HIP(hipGetLastError());
}

// K-rekey (pdl_rekey.h) of the first m keys of keys_b, `from_key64` wide, for the rank table c->rp / c->key64 hold ALREADY; the
// plan's table is in c->rk.h_table.  Queued on the stream: keys_b names the re-keyed stream afterwards and c->rk.keys the old one,
// which the caller releases once the stream has been waited for.  The values stay where they are.
static void rekey_in_place(pdl_ctx *c, uint64_t m, bool from_key64, const RkArgs &a) {
    auto &rk = c->rk;
    hipStream_t st = c->stream;
    const size_t kb = c->key64 ? 8 : 4;
    rk.keys.alloc(m * kb);
    rk.table.alloc((size_t) a.entries * kb);
    ev_begin(c, EV_REKEY);
    pdl_with_key(c->key64, [&](auto key_out) {
        using KeyOut = decltype(key_out);
        const void *h_table = rk.h_table.data();
        if (sizeof(KeyOut) == 4) {                                          // (B'^k <= 2^32: every entry fits)
            rk.h_table32.assign(rk.h_table.begin(), rk.h_table.end());
            h_table = rk.h_table32.data();
        }
        PDL_HIP(hipMemcpyAsync(rk.table.p, h_table, (size_t) a.entries * sizeof(KeyOut), hipMemcpyHostToDevice, st));
        pdl_with_key(from_key64, [&](auto key_in) {
            using KeyIn = decltype(key_in);
            pdl_rekey_stream<KeyIn, KeyOut>(st, c->keys_b.as<KeyIn>(), rk.keys.as<KeyOut>(), m, a, rk.table.as<KeyOut>());
        });
    });
    ev_end(c, EV_REKEY);
    c->keys_b.swap(rk.keys);
}

// ------------------------------------------------------------------------------------------------
// K-append (pdl_append_genomes): new genes join the dictionary that is there.
//
//   A-alpha   k_q_absent (pdl_query.h)  the new bytes against the base's letters — the only refusal that needs the device, so
//                                       it comes first: until the host has read its word the context is untouched
//   A-len     (host)                    kseq_len / k-mer offsets of the new genes; kseq_len, cost, genome ids grown to N + n
//   A-dict    k_rank / k_rank_hash + pdl_sort_pairs on the m new k-mers with the base's RankParams (gene values 0..n-1)
//   A-merge   pdl_merge_streams (pdl_append.h)   (keys_b, vals_b)[M] + the new stream -> the free half of the ping-pong; the
//                                       new genes' ids get their N there
//   tail      K-rle over the M + m stream, task layout, K-groups / K-ranges / K-cost: the build's own stages
// Option "alphabet_rekey": A-alpha comes with K-hist over the new residues; a byte the base lacks makes the union's RankParams on the
// host (rank_init_host, as a build), and in front of A-dict the base's stream is re-keyed for them (K-rekey, pdl_rekey.h), a pass of
// its own into a work buffer that then changes places with keys_b.
//
// Nothing behind K-rank reads residues, and the stream the tail starts from equals the union's sort (see pdl_append.h), so
// the context ends up as pdl_preprocess on the union leaves it.
// ------------------------------------------------------------------------------------------------
template <class KeyT>
static void append_sorted_stream(pdl_ctx *c, uint32_t n, uint64_t m, uint64_t n_res, uint32_t n_base, uint64_t m_base) {
    auto &q = c->qb;
    KeyT *k_in = q.keys_a.as<KeyT>(), *k_out = q.keys_b.as<KeyT>();
    uint32_t *v_in = q.vals_a.as<uint32_t>(), *v_out = q.vals_b.as<uint32_t>();
    ev_begin(c, EV_RANK);
    rank_new_genes<KeyT>(c, c->rp, q.res.as<uint8_t>(), q.off.as<uint64_t>(), q.koff.as<uint64_t>(), n, m, n_res, k_in, v_in);
    ev_end(c, EV_RANK);
    ev_begin(c, EV_SORT1);
    pdl_sort_pairs<KeyT>(c, k_in, k_out, v_in, v_out, m, c->rp.rank_bits, false, nullptr, 0, c->rp.key_bits == c->rp.rank_bits);
    ev_end(c, EV_SORT1);
    // what the sort ordered the base by: every bit of a rank — or, for ranks that wrapped unnoticed, the whole bytes its passes went over
    const uint32_t sorted_bits = c->rp.key_bits == c->rp.rank_bits ? 64u : std::min<uint32_t>(64u, 8u * ((c->rp.rank_bits + 7) / 8));
    const KeyT mask = sorted_bits >= 8 * sizeof(KeyT) ? (KeyT) ~(KeyT) 0 : (KeyT) (((KeyT) 1 << (sorted_bits & (8 * sizeof(KeyT) - 1))) - 1);
    ev_begin(c, EV_MERGE);
    pdl_merge_streams<KeyT>(c->stream, c->keys_b.as<KeyT>(), c->vals_b.as<uint32_t>(), (uint32_t) m_base, k_out, v_out, (uint32_t) m, n_base, mask,
                            c->scan_tmp.as<uint32_t>(), c->keys_a.as<KeyT>(), c->vals_a.as<uint32_t>());
    ev_end(c, EV_MERGE);
    c->keys_a.swap(c->keys_b); c->vals_a.swap(c->vals_b);      // the sorted stream is what keys_b / vals_b name
}

void pdl_run_append(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *genome_ids, uint32_t n, uint32_t n_new_genomes,
                    pdl_append_info *info) {
    hipStream_t st = c->stream;
    auto &q = c->qb;
    const uint32_t N0 = c->N, G0 = c->G;
    const uint64_t M0 = c->M, U0 = c->U;
    if ((uint64_t) N0 + n >= 0x7fffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu genes in the union exceed the 31-bit gene ids", (unsigned long long) N0 + n);
    const uint64_t Rq = offsets[n] - offsets[0];
    if (c->R + Rq >= 0xfffffff0ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 residues in the union need 64-bit stream positions");
    const NewGenes genes(offsets, n, c->rp.k);
    const uint64_t m = genes.M;
    if (M0 + m >= 0xfffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu k-mers in the union need 64-bit stream positions", (unsigned long long) (M0 + m));
    EventSpans<2> &spans = c->set_spans;
    spans.start(st);

    // A-alpha (and the new genes on their way to the device): the context is only read
    spans.begin();
    const bool rekey_on = c->opt_alphabet_rekey;
    constexpr size_t A_HIST = 16;             // q.ctl: [0] the smallest absent byte (k_q_absent) | [16, 272) K-hist of the new residues (rekey_on)
    q.ctl.alloc((A_HIST + 256) * sizeof(uint64_t));
    unsigned long long *d_bad = q.ctl.as<unsigned long long>();
    PDL_HIP(hipMemsetAsync(d_bad, 0, (rekey_on ? A_HIST + 256 : 1) * sizeof(uint64_t), st));
    genes.upload(c, residues);
    pdl_check_alphabet(c, q.res.as<uint8_t>(), Rq, d_bad);
    if (rekey_on && Rq) {
        hipLaunchKernelGGL(k_hist, dim3((uint32_t) std::min<uint64_t>((Rq / 64 + HIST_THREADS - 1) / HIST_THREADS + 1, 2048)), dim3(HIST_THREADS), 0, st,
                           q.res.as<uint8_t>(), Rq, d_bad + A_HIST);
        PDL_HIP(hipGetLastError());
    }
    spans.end();
    RkChange ch;
    {
        PinRead rd(c);
        const uint64_t *pb = rd.add<uint64_t>(d_bad, rekey_on ? A_HIST + 256 : 1);
        rd.sync();
        if (pb[0] && !rekey_on) pdl_fail_absent_byte(pb[0], "appended");
        if (pb[0]) {                          // the union's rank table, as a build makes it; every refusal before anything changes
            uint8_t present_union[256];
            for (int b = 0; b < 256; b++) present_union[b] = c->alpha_present[b] || pb[A_HIST + b];
            if (!rk_exact(c->rp))
                PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_append_genomes: appended byte 0x%02x is not in the base's alphabet, and the base's ranks (%u letters, "
                         "k = %u: %s) cannot be decoded into letters and written again (option alphabet_rekey); rebuild from the union",
                         256u - (uint32_t) pb[0], c->rp.base, c->rp.k, rk_why_not(c->rp));
            if (!rk_change(c->rp, c->alpha_present, present_union, c->rk.h_table, ch))
                PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_append_genomes: appended byte 0x%02x is not in the base's alphabet, and the union's ranks (%u letters, "
                         "k = %u) would be %s: the base's keys cannot be written again for them (option alphabet_rekey); rebuild from the union",
                         256u - (uint32_t) pb[0], ch.rp.base, ch.rp.k, rk_why_not(ch.rp));
        }
    }

    const SetCommit sc = commit_set_change(c, ch, M0);
    const uint32_t N1 = N0 + n, G1 = G0 + n_new_genomes;
    if (c->short_valid) short_letters_append(c->h_short_letters, G1, residues, offsets, genome_ids, n, c->rp.k);
    const uint64_t M1 = M0 + m;
    const size_t kb = c->key64 ? 8 : 4;
    // A-len: the per-gene arrays grow (k-mer counts keep their contents), the genome ids move into the context's own buffer
    c->kseq_len.grow_keep((size_t) N1 * sizeof(uint32_t), st);
    c->gene_len.grow_keep((size_t) N1 * sizeof(uint32_t), st);
    const GenomeIds ids = genome_ids_on_device(c);
    if (ids == GenomeIds::Own) c->own_gen.grow_keep((size_t) N1 * sizeof(uint32_t), st); else c->own_gen.alloc((size_t) N1 * sizeof(uint32_t));
    const uint32_t *old_gen = c->d_gen;
    pdl_extend_layout(c, genome_ids, n);                  // N, G, h_genome_of, genome rows
    c->M = M1; c->R += Rq;
    c->d_gen = c->own_gen.as<uint32_t>(); c->d_res = nullptr; c->d_off = nullptr;          // (nothing behind K-rank reads residues or offsets)
    if (m) {
        c->keys_a.alloc(M1 * kb); c->vals_a.alloc(M1 * sizeof(uint32_t));
        q.keys_a.alloc(m * kb); q.keys_b.alloc(m * kb); q.vals_a.alloc(m * 4); q.vals_b.alloc(m * 4);
        c->scan_tmp.alloc(pdl_merge_split_words(M1) * sizeof(uint32_t));
    }
    rebuild_behind_sort(c, sc.ri, M1, N1, G1, [&] {        // (behind the clearing, as ever: the new genes' tails of the per-gene arrays, A-dict, A-merge)
        PDL_HIP(hipMemcpyAsync(c->kseq_len.as<uint32_t>() + N0, q.kseq.p, n * 4ull, hipMemcpyDeviceToDevice, st));
        PDL_HIP(hipMemcpyAsync(c->gene_len.as<uint32_t>() + N0, genes.len.data(), n * 4ull, hipMemcpyHostToDevice, st));
        if (ids == GenomeIds::Own) {
            PDL_HIP(hipMemcpyAsync(c->own_gen.as<uint32_t>() + N0, c->h_genome_of.data() + N0, n * 4ull, hipMemcpyHostToDevice, st));
        } else if (ids == GenomeIds::Ingest) {
            PDL_HIP(hipMemcpyAsync(c->own_gen.p, old_gen, (size_t) N0 * 4, hipMemcpyDeviceToDevice, st));
            PDL_HIP(hipMemcpyAsync(c->own_gen.as<uint32_t>() + N0, c->h_genome_of.data() + N0, n * 4ull, hipMemcpyHostToDevice, st));
        } else {
            PDL_HIP(hipMemcpyAsync(c->own_gen.p, c->h_genome_of.data(), (size_t) N1 * 4, hipMemcpyHostToDevice, st));
        }
        if (ch.rekey) rekey_in_place(c, M0, sc.key64_before, ch.args);
        if (m) pdl_with_key(c->key64, [&](auto key) { append_sorted_stream<decltype(key)>(c, n, m, Rq, N0, M0); });
    });
    const float rank_ms = ev_ms(c, EV_RANK), sort_ms = ev_ms(c, EV_SORT1), merge_ms = ev_ms(c, EV_MERGE);
    c->tm.rank_ms = rank_ms; c->tm.sort_rank_ms = sort_ms + merge_ms + c->last_rekey.rekey_ms;
    if (info) {
        info->residues = Rq; info->kmer_occurrences = m;
        info->records = c->U - U0;            // (a record belongs to one gene: the base's records are all still there)
        info->rank_sort_ms = rank_ms + sort_ms; info->merge_ms = merge_ms; info->device_ms = c->tm.preprocess_total_ms;
    }
}

// ------------------------------------------------------------------------------------------------
// K-remove (pdl_remove_genomes): the genes of some genomes leave the dictionary that is there.
//
//   R-map      scan over the genes (pdl_remove.h)      new gene ids, the per-gene arrays closed up, genome ids renumbered
//   R-compact  pdl_compact_stream (pdl_remove.h)       (keys_b, vals_b)[M] without the leaving genes' k-mers -> the free half of the
//   + R-alpha                                          ping-pong; the digits of the keys that stay
//   -- the host's one read: k-mers left (none: PDL_ERR_EMPTY), digits seen (one missing: PDL_ERR_UNSUPPORTED).  Up to here the
//      context is only read: R-map writes work buffers, the compaction the half of the ping-pong nobody reads --
//   tail       K-rle over the M' stream, task layout, K-groups / K-ranges / K-cost: the build's own stages
//
// The rank table depends on the set's alphabet only (library.cpp:96-119).  A polynomial rank with an exact B^k is
// sum v[c_i] * B^(k-1-i) with dense digits v, so the digits of the keys that stay name letters the remaining set holds; when
// they cover all B letters the remaining set's table is the context's, and the stream the tail starts from is the one
// pdl_preprocess would sort for the remaining set (see pdl_remove.h).  A letter that survives only in genes shorter than k
// cannot be seen this way: that removal is refused although a rebuild would have agreed.
// Option "alphabet_rekey", on a context built with it: c->h_short_letters holds exactly those letters, so the remaining alphabet is
// known — the digits seen plus the short genes' letters of the genomes that stay.  The context's: the removal goes through.
// Smaller: the tail starts with K-rekey (pdl_rekey.h) of the compacted stream for the remaining set's RankParams.
// ------------------------------------------------------------------------------------------------
void pdl_run_remove(pdl_ctx *c, const uint32_t *genomes, uint32_t count, pdl_remove_info *info) {
    hipStream_t st = c->stream;
    auto &r = c->rm;
    const uint32_t N0 = c->N, G0 = c->G, G1 = G0 - count;
    const uint64_t M0 = c->M, U0 = c->U;
    if (!rk_exact(c->rp))                     // a key decodes into letters when it is the polynomial itself
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_remove_genomes: the ranks of this set (%u letters, k = %u: %s) cannot be decoded into letters, so the remaining "
                 "set cannot be shown to have the same alphabet; rebuild from the remaining genes", c->rp.base, c->rp.k, rk_why_not(c->rp));
    // genome ids of the remaining set: the order they have, closed up
    std::vector<uint32_t> gmap((size_t) G0, 0u);
    for (uint32_t i = 0; i < count; i++) gmap[genomes[i]] = RM_GONE;
    for (uint32_t g = 0, next = 0; g < G0; g++) if (gmap[g] != RM_GONE) gmap[g] = next++;
    EventSpans<2> &spans = c->set_spans;
    spans.start(st);

    // R-map, R-compact, R-alpha: the context is only read
    spans.begin();
    r.ctl.alloc(PDL_RM_WORDS * sizeof(uint64_t));
    uint64_t *d_ctl = r.ctl.as<uint64_t>();
    hipLaunchKernelGGL(k_zero_u64, dim3(1), dim3(256), 0, st, d_ctl, (size_t) PDL_RM_WORDS);
    r.gmap.alloc((size_t) G0 * 4);
    PDL_HIP(hipMemcpyAsync(r.gmap.p, gmap.data(), (size_t) G0 * 4, hipMemcpyHostToDevice, st));
    const uint32_t *d_gen = c->d_gen;
    if (genome_ids_on_device(c) == GenomeIds::Callers) {
        r.gen_in.alloc((size_t) N0 * 4);
        PDL_HIP(hipMemcpyAsync(r.gen_in.p, c->h_genome_of.data(), (size_t) N0 * 4, hipMemcpyHostToDevice, st));
        d_gen = r.gen_in.as<uint32_t>();
    }
    r.new_id.alloc((size_t) N0 * 4); r.kseq.alloc((size_t) N0 * 4); r.gen.alloc((size_t) N0 * 4); r.glen.alloc((size_t) N0 * 4);
    r.tile.alloc(pdl_remove_tiles(M0) * sizeof(uint32_t));
    const size_t kb = c->key64 ? 8 : 4;
    c->keys_a.alloc(M0 * kb); c->vals_a.alloc(M0 * sizeof(uint32_t));     // (the free half: after an append it is the smaller one)
    scan_and_apply(c, N0, RmStays{d_gen, r.gmap.as<uint32_t>()},
                   RmMapApply{d_gen, r.gmap.as<uint32_t>(), c->kseq_len.as<uint32_t>(), c->gene_len.as<uint32_t>(), r.new_id.as<uint32_t>(), r.gen.as<uint32_t>(),
                              r.kseq.as<uint32_t>(), r.glen.as<uint32_t>(), reinterpret_cast<unsigned long long *>(d_ctl + PDL_RM_GONE_RESIDUES)},
                   d_ctl + PDL_RM_GENES);
    pdl_with_key(c->key64, [&](auto key) {
        using KeyT = decltype(key);
        pdl_compact_stream<KeyT>(st, c->keys_b.as<KeyT>(), c->vals_b.as<uint32_t>(), r.new_id.as<uint32_t>(), M0, r.tile.as<uint32_t>(), c->keys_a.as<KeyT>(),
                                 c->vals_a.as<uint32_t>(), rm_digits(c->rp.k, c->rp.base), reinterpret_cast<uint32_t *>(d_ctl + PDL_RM_SEEN), d_ctl + PDL_RM_KMERS);
    });
    spans.end();
    // the host's side of it while the device works: the genome ids of the genes that stay
    std::vector<uint32_t> genome_of;
    genome_of.reserve(N0);
    for (uint32_t i = 0; i < N0; i++) if (gmap[c->h_genome_of[i]] != RM_GONE) genome_of.push_back(gmap[c->h_genome_of[i]]);
    const uint32_t N1 = (uint32_t) genome_of.size();
    uint64_t M1 = 0, gone_residues = 0;
    bool digit_missing = false;
    RkChange ch;
    {
        PinRead rd(c);
        const uint64_t *pc = rd.add<uint64_t>(d_ctl, PDL_RM_WORDS);
        const uint32_t *lbe = lookback_error_word(c, rd);
        rd.sync();
        lookback_check(c, lbe);
        if (pc[PDL_RM_GENES] != N1) PDL_FAIL(PDL_ERR_DEVICE, "pdl_remove_genomes: %llu genes stay on the device, %u on the host", (unsigned long long) pc[PDL_RM_GENES], N1);
        M1 = pc[PDL_RM_KMERS]; gone_residues = pc[PDL_RM_GONE_RESIDUES];
        if (M1 == 0) PDL_FAIL(PDL_ERR_EMPTY, "no gene is at least k=%u residues long: the dictionary is empty", c->rp.k);
        const uint32_t *seen = reinterpret_cast<const uint32_t *>(pc + PDL_RM_SEEN);
        for (uint32_t d = 0; d < c->rp.base; d++) {
            if (seen[d]) continue;
            if (c->opt_alphabet_rekey) { digit_missing = true; break; }
            int letter = 0;
            for (int b = 0; b < 256; b++) if (c->alpha_present[b] && c->rp.rank_values[b] == d) { letter = b; break; }
            PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_remove_genomes: no k-mer of the remaining genes holds the letter 0x%02x%s%c%s: without it the remaining set has "
                     "another rank table (this check is conservative: the letter may survive in a gene shorter than k=%u); rebuild from the remaining genes",
                     letter, letter >= 0x20 && letter < 0x7f ? " ('" : "", letter >= 0x20 && letter < 0x7f ? (char) letter : ' ',
                     letter >= 0x20 && letter < 0x7f ? "')" : "", c->rp.k);
        }
        if (digit_missing) {
            if (!c->short_valid)
                PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_remove_genomes: no k-mer of the remaining genes holds every letter of the alphabet, and the letters of genes "
                         "shorter than k=%u are not known: option alphabet_rekey was not set when the context was built (set it before pdl_preprocess); "
                         "rebuild from the remaining genes", c->rp.k);
            // the remaining alphabet, exactly: every residue lies in a k-mer or in a gene shorter than k
            uint8_t in_short[256], present_left[256];
            short_letters_staying(c->h_short_letters, gmap, in_short);
            for (int b = 0; b < 256; b++) present_left[b] = c->alpha_present[b] && (seen[c->rp.rank_values[b]] || in_short[b]);
            if (!rk_change(c->rp, c->alpha_present, present_left, c->rk.h_table, ch))      // (cannot happen: fewer letters than an exact table has)
                PDL_FAIL(PDL_ERR_UNSUPPORTED, "pdl_remove_genomes: the remaining set's ranks (%u letters, k = %u) would be %s", ch.rp.base, ch.rp.k, rk_why_not(ch.rp));
        }
    }

    const SetCommit sc = commit_set_change(c, ch, M1);
    if (c->short_valid) short_letters_remove(c->h_short_letters, gmap, G1);
    c->keys_a.swap(c->keys_b); c->vals_a.swap(c->vals_b);      // the sorted stream is what keys_b / vals_b name
    c->kseq_len.swap(r.kseq); c->gene_len.swap(r.glen);
    c->own_gen.swap(r.gen);                                     // the context owns the ids from here on, as after an append
    pdl_replace_layout(c, std::move(genome_of));          // N, G, h_genome_of, genome rows
    c->M = M1; c->R -= gone_residues;
    c->d_gen = c->own_gen.as<uint32_t>(); c->d_res = nullptr; c->d_off = nullptr;          // (nothing behind K-rank reads residues or offsets)
    rebuild_behind_sort(c, sc.ri, M1, N1, G1, [&] { if (ch.rekey) rekey_in_place(c, M1, sc.key64_before, ch.args); });      // (the compacted stream is in place)
    const float ms0 = spans.ms(0);
    c->tm.sort_rank_ms = ms0 + c->last_rekey.rekey_ms;
    if (info) {
        info->sequences = N0 - N1; info->residues = gone_residues; info->kmer_occurrences = M0 - M1;
        info->records = U0 - c->U;            // (a record belongs to one gene: the records of the genes that stay are all still there)
        info->compact_ms = ms0; info->device_ms = c->tm.preprocess_total_ms;
    }
}

void pdl_run_preprocess(pdl_ctx *c, int kvalue, bool only_complexity) {
    hipStream_t st = c->stream;
    ev_begin(c, EV_PRE_TOTAL);
    c->short_valid = false;
    stage_alphabet_and_lengths(c, kvalue, only_complexity);
    pdl_with_key(c->key64, [&](auto key) { dictionary_pipeline<decltype(key)>(c, only_complexity); });
    ev_end(c, EV_PRE_TOTAL);
    PDL_HIP(hipStreamSynchronize(st));
    if (c->opt_alphabet_rekey) {                    // the table is the context's own from here on, on the host: a few words a genome
        short_letters_fetch(c->h_short_letters, c->rk.short_letters.p, c->G);
        c->short_valid = true;
    }
    c->tm.hist_ms = ev_ms(c, EV_HIST);
    c->tm.rank_ms = ev_ms(c, EV_RANK);
    c->tm.sort_rank_ms = ev_ms(c, EV_SORT1);
    c->tm.dict_ms = ev_ms(c, EV_DICT);
    c->tm.sort_seq_ms = only_complexity ? 0.f : ev_ms(c, EV_SORT2);
    c->tm.ranges_ms = only_complexity ? 0.f : ev_ms(c, EV_RANGES);
    c->tm.preprocess_total_ms = ev_ms(c, EV_PRE_TOTAL);
    c->tm.dist_begin_ms = c->tm.dist_finish_ms = 0.f;
}

// ------------------------------------------------------------------------------------------------
// Multi-GPU build (include/pandelos_amd.h, pdl_dist_*).  Every GPU ranks all k-mers (the input is shared), keeps the
// ones of its rank interval, and sorts + dedups those: its run of the dictionary.  The caller all-gathers the runs; the
// concatenation in rank order is the dictionary of library.cpp:270-287, so no merge is needed.
// ------------------------------------------------------------------------------------------------
template <class KeyT>
static void dist_slice_pipeline(pdl_ctx *c) {
    hipStream_t st = c->stream;
    const uint64_t M = c->M;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    const uint32_t W = c->world, me = c->rank;
    // 1. every k-mer's rank, and as a by-product the k-mers per bin of the rank space (top DIST_BIN_BITS bits of a rank)
    ev_begin(c, EV_RANK);
    // (the bins go over the bits a rank can occupy; where ranks wrapped unnoticed AND the reference's sort goes over fewer bytes than
    // they fill, its dictionary is ordered by the low bytes only: intervals of the high bits cannot reproduce that across GPUs)
    if (c->rp.key_bits != c->rp.rank_bits && c->rp.rank_bits <= 56)
        PDL_FAIL(PDL_ERR_UNSUPPORTED, "k-mer ranks wrap past 2^64 unnoticed by the reference's overflow test and its sort covers %u bits of them: one GPU reproduces that order, several do not", c->rp.rank_bits);
    const uint32_t shift = c->rp.key_bits > DIST_BIN_BITS ? c->rp.key_bits - DIST_BIN_BITS : 0;
    c->scratch2.alloc(std::max<size_t>(c->scratch2.bytes, DIST_BINS * sizeof(uint32_t)));
    uint32_t *d_bins = c->scratch2.as<uint32_t>();
    PDL_HIP(hipMemsetAsync(d_bins, 0, DIST_BINS * sizeof(uint32_t), st));
    stage_rank<KeyT>(c, d_bins, shift);
    ev_end(c, EV_RANK);
    std::vector<uint64_t> pre(DIST_BINS + 1, 0);
    {
        PinRead rd(c);
        const uint32_t *pb = rd.add<uint32_t>(d_bins, DIST_BINS);
        rd.sync();
        for (uint32_t b = 0; b < DIST_BINS; b++) pre[b + 1] = pre[b] + pb[b];
    }
    if (pre[DIST_BINS] != M) PDL_FAIL(PDL_ERR_DEVICE, "interval histogram counts %llu k-mers, the stream holds %llu", (unsigned long long) pre[DIST_BINS], (unsigned long long) M);
    // cut w = first bin whose exclusive prefix reaches w * M / W: the same on every rank (function of the input only)
    auto cut = [&](uint32_t w) -> uint32_t {
        if (w == 0) return 0;
        if (w >= W) return DIST_BINS;
        const uint64_t target = (uint64_t) ((unsigned __int128) M * w / W);
        return (uint32_t) (std::lower_bound(pre.begin(), pre.end() - 1, target) - pre.begin());
    };
    const uint32_t b_lo = cut(me), b_hi = cut(me + 1);
    const uint64_t m_own = pre[b_hi] - pre[b_lo];
    c->M_slice = m_own;
    c->dist_tail = -1;                      // the last rank whose interval holds k-mers: it holds the dictionary's last record
    for (uint32_t w = 0; w < W; w++) if (pre[cut(w + 1)] > pre[cut(w)]) c->dist_tail = (int) w;
    // 3. this rank's k-mers, in stream order (the sort below is stable: equal ranks keep ascending gene order)
    KeyT *sel_k = c->keys_b.as<KeyT>();
    uint32_t *sel_v = c->vals_b.as<uint32_t>();
    scan_and_apply(c, M, SelFlag<KeyT>{c->keys_a.as<KeyT>(), shift, b_lo, b_hi},
                   SelApply<KeyT>{c->keys_a.as<KeyT>(), c->vals_a.as<uint32_t>(), sel_k, sel_v}, d_scal + PDL_CTL_SELECT_TOTAL);
    // 4. sort + dedup 1/W of the stream; the group-head flag rides in bit 31 of the count
    c->U_slice = 0;
    if (m_own) {
        KeyT *keys_in = sel_k, *keys_out = c->keys_a.as<KeyT>();
        uint32_t *vals_in = sel_v, *vals_out = c->vals_a.as<uint32_t>();
        stage_sort_and_dedup<KeyT>(c, keys_in, keys_out, vals_in, vals_out, m_own);
        // The reference folds the dictionary's LAST record into the group before it (library.cpp:300-306).  That record is in
        // the run of the last rank with k-mers, and so is the group it joins whenever that run has two records or more (groups
        // never straddle runs): the fold is made here, on the run, and travels with it (it is idempotent: the finish that
        // looks at the gathered dictionary finds nothing left to do; a last run of ONE record is left to that finish).
        if ((int) me == c->dist_tail)
            hipLaunchKernelGGL(k_fold_last_record, dim3(1), dim3(1024), 0, st, c->post.as<uint2>(), c->recpos.as<uint32_t>(), d_scal + PDL_CTL_RECORDS);
        // every genome's lookups inside this run (groups never straddle runs), as the reference counts them and above the
        // diagonal: summed over the ranks the former are "Genome g cost" (exact when the fold above was made), the latter the
        // weights of the genome deal
        GroupPlan gp = group_tiles_plan(c, c->post.as<uint2>(), m_own, d_scal + PDL_CTL_RECORDS);
        gp.a.counters = reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_SLICE_COUNTERS);    // (scratch words: the real counters come from the finish)
        gp.a.g_full = reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_GCOST);           // scratch here, cleared again by the finish
        gp.a.g_upper = gp.a.g_full + c->G;
        launch_group_costs<true, false>(c, gp.a, gp.grid);
        ev_end(c, EV_DICT);
    } else {
        c->post.alloc(16);
    }
}

void pdl_run_dist_begin(pdl_ctx *c, int kvalue) {
    hipStream_t st = c->stream;
    ev_begin(c, EV_PRE_TOTAL);
    ev_begin(c, EV_DIST_BEGIN);
    c->dist = true; c->dist_stage = DistStage::none; c->post_ext = nullptr;
    stage_alphabet_and_lengths(c, kvalue, false);
    pdl_with_key(c->key64, [&](auto key) { dist_slice_pipeline<decltype(key)>(c); });
    ev_end(c, EV_DIST_BEGIN);
    c->h_run_weights.assign(c->G, 0);
    c->h_run_costs.assign(c->G, 0);
    c->dist_sender = false;
    if (c->M_slice) {
        PinRead rd(c);
        const uint64_t *pu = rd.add<uint64_t>(c->scalars.as<uint64_t>() + PDL_CTL_RECORDS, 1);
        const uint64_t *pw = rd.add<uint64_t>(c->scalars.as<uint64_t>() + PDL_CTL_GCOST + c->G, c->G);
        const uint64_t *pf = rd.add<uint64_t>(c->scalars.as<uint64_t>() + PDL_CTL_GCOST, c->G);
        rd.sync();
        c->U_slice = pu[0];
        c->h_run_weights.assign(pw, pw + c->G);
        c->h_run_costs.assign(pf, pf + c->G);
    } else {
        PDL_HIP(hipStreamSynchronize(st));
    }
    c->tm.hist_ms = ev_ms(c, EV_HIST);
    c->tm.rank_ms = ev_ms(c, EV_RANK);
    c->tm.sort_rank_ms = c->M_slice ? ev_ms(c, EV_SORT1) : 0.f;
    c->tm.dict_ms = c->M_slice ? ev_ms(c, EV_DICT) : 0.f;
    c->tm.dist_begin_ms = ev_ms(c, EV_DIST_BEGIN);
    c->dist_stage = DistStage::slice_built;
}

// longest-processing-time assignment, deterministic (ties: lower genome id first, then lower rank)
static void lpt_owner(const std::vector<uint64_t> &w, uint32_t world, std::vector<uint32_t> &owner) {
    const uint32_t G = (uint32_t) w.size();
    std::vector<uint32_t> order(G);
    for (uint32_t g = 0; g < G; g++) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return w[a] > w[b]; });
    std::vector<uint64_t> load(world, 0);
    owner.assign(G, 0);
    for (uint32_t g : order) {
        uint32_t best = 0;
        for (uint32_t r = 1; r < world; r++) if (load[r] < load[best]) best = r;
        owner[g] = best;
        load[best] += w[g] + 1;          // (+1: genomes without any lookup still spread over the ranks)
    }
}

// genomes -> ranks by longest-processing-time on each genome's lookups above the diagonal (`weights`; nullptr: h_upper_cost
// holds them already); the deal goes to the device
static void dist_deal_genomes(pdl_ctx *c, const uint64_t *weights) {
    if (weights) c->h_upper_cost.assign(weights, weights + c->G);
    lpt_owner(c->h_upper_cost, c->world, c->h_owner);
    c->shard.clear();
    for (uint32_t g = 0; g < c->G; g++) if (c->h_owner[g] == c->rank) c->shard.push_back(g);
    c->shard_set = true;
    c->dict_shard = c->shard;
    c->tasks_ready = false;                 // (the task layout is prepared behind the launches of the two passes, or by the finish)
    c->owner_of_genome.alloc((size_t) c->G * 4);
    PDL_HIP(hipMemcpyAsync(c->owner_of_genome.p, c->h_owner.data(), (size_t) c->G * 4, hipMemcpyHostToDevice, c->stream));
}

// what a gathered dictionary of `total` records is refused for
static void check_dictionary_total(uint64_t total) {
    if (total == 0) PDL_FAIL(PDL_ERR_EMPTY, "empty dictionary");
    if (total >= 0xfffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "a dictionary of %llu records needs 64-bit record indices", (unsigned long long) total);
}

// the pinned scratch a finish uploads control words from (rewritten only by the next PinRead, which comes after a sync)
static uint64_t *pinned_words(pdl_ctx *c) {
    if (!c->pin) PDL_FAIL(PDL_ERR_DEVICE, "pinned scratch missing");
    return reinterpret_cast<uint64_t *>(c->pin);
}

// the tail of both finishes; ranges_ms: what the sender path spent between begin and finish
static void dist_finish_tail(pdl_ctx *c, float ranges_ms) {
    ev_end(c, EV_DIST_FINISH); ev_end(c, EV_PRE_TOTAL);
    c->tm.dist_finish_ms = close_range_timings(c, EV_DIST_FINISH);
    c->tm.preprocess_total_ms = c->tm.dist_begin_ms + ranges_ms + c->tm.dist_finish_ms;
    c->dist_stage = DistStage::adopted;
}

void pdl_run_dist_finish(pdl_ctx *c, uint64_t total, const uint64_t *weights) {
    hipStream_t st = c->stream;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    ev_begin(c, EV_DIST_FINISH);
    check_dictionary_total(total);
    // the record count of the whole dictionary goes where the kernels expect it (PDL_CTL_RECORDS); the other counters and the
    // per-genome words restart
    uint64_t *h_u = pinned_words(c); h_u[0] = total;
    PDL_HIP(hipMemcpyAsync(d_scal + PDL_CTL_RECORDS, h_u, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // (BAD_OFFSETS .. KSEQ_NMIN belong to K-len and stay: bad-offsets flag, kseq sums, M)
    clear_ctl(c, PDL_CTL_FREE_1, PDL_CTL_RANGES);
    clear_ctl(c, PDL_CTL_MIRRORED, PDL_CTL_LAST);
    clear_genome_words(c);
    // the deal goes by the caller's sum of the runs' weights, or — without one — by an exact pass over the gathered dictionary first
    c->h_upper_cost.assign(c->G, 0);
    if (!weights) {
        c->scratch2.alloc(std::max<size_t>(c->scratch2.bytes, ((size_t) c->G + 2) * sizeof(uint64_t)));
        PDL_HIP(hipMemsetAsync(c->scratch2.p, 0, ((size_t) c->G + 2) * sizeof(uint64_t), st));
        GroupPlan gp = group_tiles_plan(c, c->post_ext, total, nullptr);
        gp.a.counters = c->scratch2.as<unsigned long long>() + c->G;
        gp.a.g_upper = c->scratch2.as<unsigned long long>();
        gp.a.g_full = reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_GCOST);     // (scratch: the K-cost words are cleared below)
        // (the fold of the last record is not applied yet: as with the callers' weights, these numbers only balance)
        launch_group_costs<true, false>(c, gp.a, gp.grid);
        PinRead rd(c);
        const uint64_t *pu = rd.add<uint64_t>(gp.a.g_upper, c->G);
        rd.sync();
        c->h_upper_cost.assign(pu, pu + c->G);
        clear_genome_words(c);
    }
    dist_deal_genomes(c, weights);
    c->seq_in_shard.alloc(c->N);
    hipLaunchKernelGGL(k_genes_of_rank, dim3((c->N + 255) / 256), dim3(256), 0, st, c->d_gen, c->owner_of_genome.as<uint32_t>(), c->rank, c->N,
                       c->seq_in_shard.as<uint8_t>());
    stage_ranges_and_costs(c, total, 2, false);
    dist_finish_tail(c, 0.f);
}

// ---- sender-built range lists ----------------------------------------------------------------------------------------------------
// pdl_run_dist_finish makes every rank walk the WHOLE gathered dictionary twice (COUNT, WRITE) to find the ranges of its own
// genes: work that does not shrink with the number of ranks.  Groups never straddle runs, so everything a range tuple says —
// the gene, where its postings start, how many there are, the gene's own count — is known to the rank that holds the run, up to
// the run's place in the gathered array, which the record counts give.  Here a rank makes the tuples of ALL genes in its run
// (1/world of the records, no "is this gene mine" per record), files them by the rank that owns the gene (one stable radix
// pass on the owner byte: record order survives, so a gene's ranges still arrive in (rank, gene) order when the sources are
// concatenated in rank order), and the owners sort what they receive by gene.
bool pdl_run_dist_ranges(pdl_ctx *c, const uint64_t *run_records, const uint64_t *weights, const uint64_t *costs) {
    hipStream_t st = c->stream;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    const uint32_t W = c->world, me = c->rank;
    uint64_t total = 0, base = 0;
    int tail = -1;
    for (uint32_t r = 0; r < W; r++) { if (r < me) base += run_records[r]; total += run_records[r]; if (run_records[r]) tail = (int) r; }
    if (run_records[me] != c->U_slice) PDL_FAIL(PDL_ERR_ARGUMENT, "run_records[%u] = %llu, this rank's run holds %llu records", me, (unsigned long long) run_records[me], (unsigned long long) c->U_slice);
    check_dictionary_total(total);
    c->dist_total = total; c->run_base = base;
    c->h_tuple_counts.assign(W, 0);
    c->dist_out_keys = nullptr; c->dist_out_ranges = nullptr; c->dist_out_total = 0;
    c->dist_run_counters[0] = c->dist_run_counters[1] = c->dist_run_counters[2] = 0;
    // Not this way (every rank decides the same: all of it is a function of the input and of the record counts): packed ranges
    // need gene ids of 22 bits, the owner a byte; a last run of ONE record has not been folded (the group it joins is in
    // another rank's run).
    c->dist_sender = c->N < (1u << 22) && W <= 256 && tail == c->dist_tail && (run_records[tail] >= 2 || total == 1);
    if (!c->dist_sender) return false;
    ev_begin(c, EV_DIST_RANGES);
    dist_deal_genomes(c, weights);
    c->h_genome_cost.assign(costs, costs + c->G);       // exact: the fold was made before the runs were counted
    c->seq_owner.alloc(c->N);
    hipLaunchKernelGGL(k_gene_owner, dim3((c->N + 255) / 256), dim3(256), 0, st, c->d_gen, c->owner_of_genome.as<uint32_t>(), c->N, c->seq_owner.as<uint8_t>());
    const uint64_t n_run = c->U_slice;
    if (n_run) {
        clear_ctl(c, PDL_CTL_RANGES, PDL_CTL_RANGES);
        clear_ctl(c, PDL_CTL_COUNTERS, PDL_CTL_REPEATS);
        GroupPlan gp = group_tiles_plan(c, c->post.as<uint2>(), n_run, d_scal + PDL_CTL_RECORDS);      // (the run's record count is still where K-rle left it)
        gp.a.cost = c->cost.as<unsigned long long>();
        gp.a.counters = reinterpret_cast<unsigned long long *>(d_scal + PDL_CTL_COUNTERS);
        gp.a.pos_base = (uint32_t) base;
        RangeBufs b{};
        const uint64_t n_t = count_then_write(c, gp.a, gp.grid, 1, range_plan(c, 1, true), false, b);
        if (n_t) {
            hipLaunchKernelGGL(k_owner_keys, dim3((uint32_t) std::min<uint64_t>((n_t + 255) / 256, (uint64_t) c->cus * 16)), dim3(256), 0, st, b.k2a, d_scal + PDL_CTL_RANGES, c->seq_owner.as<uint8_t>());
            pdl_sort_pairs<uint32_t, unsigned long long>(c, b.k2a, b.k2b, b.pay_a, b.pay_b, n_t, 32, false, nullptr, 24, true);      // -> (k2b, pay_b), by destination
            c->tuple_off.alloc(((size_t) W + 1) * sizeof(uint32_t));
            hipLaunchKernelGGL(k_seq_offsets, dim3((W + 1 + 255) / 256), dim3(256), 0, st, b.k2b, d_scal + PDL_CTL_RANGES, W, c->tuple_off.as<uint32_t>(), 24u, 0xffu);
            PDL_HIP(hipGetLastError());
            c->dist_out_keys = b.k2b; c->dist_out_ranges = b.pay_b; c->dist_out_total = n_t;
        }
        PinRead rd(c);
        const uint64_t *pc = rd.add<uint64_t>(d_scal + PDL_CTL_COUNTERS, PDL_CTL_REPEATS - PDL_CTL_COUNTERS + 1);
        const uint32_t *po = n_t ? rd.add<uint32_t>(c->tuple_off.as<uint32_t>(), W + 1) : nullptr;
        rd.sync();
        c->dist_run_counters[0] = pc[PDL_CTL_SHARED - PDL_CTL_COUNTERS]; c->dist_run_counters[1] = pc[PDL_CTL_GROUPS - PDL_CTL_COUNTERS];
        c->dist_run_counters[2] = pc[PDL_CTL_REPEATS - PDL_CTL_COUNTERS];
        if (po) {
            for (uint32_t r = 0; r < W; r++) c->h_tuple_counts[r] = po[r + 1] - po[r];
            if (po[W] != n_t) PDL_FAIL(PDL_ERR_DEVICE, "range tuples: %llu made, %u filed", (unsigned long long) n_t, po[W]);
        }
    }
    ev_end(c, EV_DIST_RANGES);
    PDL_HIP(hipStreamSynchronize(st));
    c->tm.dist_ranges_ms = ev_ms(c, EV_DIST_RANGES);
    return true;
}

// the owner's side: the gathered dictionary is adopted, the received tuples (source-rank major) are sorted by gene
void pdl_run_dist_finish_ranges(pdl_ctx *c, uint64_t total, uint32_t *d_keys, unsigned long long *d_ranges, uint64_t n_in, const uint64_t *sums) {
    hipStream_t st = c->stream;
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    ev_begin(c, EV_DIST_FINISH);
    if (total != c->dist_total) PDL_FAIL(PDL_ERR_ARGUMENT, "the gathered dictionary holds %llu records, the runs add up to %llu", (unsigned long long) total, (unsigned long long) c->dist_total);
    if (n_in >= 0xfffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 range tuples for one rank");
    // the tuples come from other processes: nothing of this context is touched before they have been looked at
    if (n_in) {
        uint64_t own_genes = 0;
        for (uint32_t g : c->shard) own_genes += c->h_genome_row_off[g + 1] - c->h_genome_row_off[g];
        if (own_genes == 0) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_dist_preprocess_finish_ranges: %llu range tuples received by a rank that owns no gene", (unsigned long long) n_in);
        clear_ctl(c, PDL_CTL_FREE_1, PDL_CTL_FREE_1);
        hipLaunchKernelGGL(k_tuple_check, dim3((uint32_t) ((n_in + 255) / 256)), dim3(256), 0, st, d_keys, d_ranges, (uint32_t) n_in, c->seq_owner.as<uint8_t>(), c->N,
                           c->rank, (uint32_t) total, d_scal + PDL_CTL_FREE_1);
        PDL_HIP(hipGetLastError());
        PinRead rd(c);
        const uint64_t *bad = rd.add<uint64_t>(d_scal + PDL_CTL_FREE_1, 1);
        rd.sync();
        if (*bad) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_dist_preprocess_finish_ranges: %llu of the %llu received range tuples do not name this rank and a gene of its genomes (%u genes), or reach past the %llu records of the dictionary; begin the build again (pdl_dist_preprocess_begin)",
                           (unsigned long long) *bad, (unsigned long long) n_in, c->N, (unsigned long long) total);
    }
    uint64_t *h_u = pinned_words(c);
    h_u[PDL_CTL_RECORDS] = total; h_u[PDL_CTL_FREE_1] = 0; h_u[PDL_CTL_RANGES] = n_in;
    PDL_HIP(hipMemcpyAsync(d_scal + PDL_CTL_RECORDS, h_u, (PDL_CTL_RANGES - PDL_CTL_RECORDS + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    clear_kseq_stats(c);
    clear_ctl(c, PDL_CTL_MIRRORED, PDL_CTL_LAST);
    clear_genome_words(c);
    clear_gene_costs(c);
    ev_begin(c, EV_SORT2);
    const RangeBufs b = carve_ranges(c, RANGES_RECEIVED, std::max<uint64_t>(n_in, 1), d_keys, d_ranges);
    c->dist_out_keys = nullptr; c->dist_out_ranges = nullptr; c->dist_out_total = 0;
    // the gene bits only (gene ids have 22 bits at most: the owner byte lies above every digit)
    sort_ranges_by_gene(c, b, n_in, nullptr, 0, 0xffffffu);
    // the k-mer statistics of the genes (the per-gene costs are all zero here: what it adds up per genome is not used)
    launch_genome_cost(c, PDL_CTL_KSEQ_SUM, PDL_CTL_KSEQ_MAX);
    if (!c->tasks_ready) pdl_prepare_tasks(c);           // host work + small uploads while the device sorts
    { PinRead rd(c); closing_read(c, rd, PDL_CTL_KSEQ_NMIN + 1); }
    c->U = total; c->Ushared = sums[0]; c->NG = sums[1]; c->Urepeat = sums[2];
    c->P = 0;
    for (uint32_t g : c->shard) c->P += c->h_genome_cost[g];
    c->costs_ready = true;                   // per genome, from the runs' counts; per gene: not kept by this build (pdl_sequence_costs says so)
    dist_finish_tail(c, c->tm.dist_ranges_ms);
}
