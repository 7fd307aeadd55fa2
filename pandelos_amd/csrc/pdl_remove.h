// pdl_remove.h — K-remove: the genes of some genomes leave the sorted k-mer stream of a context (pdl_remove_genomes,
// include/pandelos_amd.h), included from pdl_dict.hip, whose stages the removal runs behind it.
//
// The stream (keys_b, vals_b)[M] is sorted by (rank, input position) (pdl_sort_pairs is a stable LSD sort over the stream K-rank
// writes gene by gene).  Taking elements out keeps the order of the others, and renumbering the genes that stay monotonically
// keeps "input position" meaning what it meant: what is left is the stream pdl_preprocess would sort for the remaining set —
// as long as the rank table is the same, which R-alpha proves or the call is refused.
//
//   R-map      RmStays / RmMapApply through scan_and_apply over the N genes: new_id[gene] (RM_GONE for one that leaves), the
//              compacted kseq_len / gene_len / genome ids (renumbered through gmap[G]), the residues that leave
//   R-compact  k_rm_count -> k_scan_tile_scan -> k_rm_compact: the stable compaction of the stream into the free half of the
//              ping-pong, every value rewritten to new_id[value]
//   R-alpha    inside k_rm_compact, on the keys it keeps: which base-B digits occur (polynomial ranks with an exact B^k only)
//
// A tile is RM_TILE consecutive elements; wave w of the workgroup takes the RM_ITEMS * 64 elements [w * 512, (w + 1) * 512) of
// it in RM_ITEMS rounds of 64 consecutive elements (one 256- or 512-byte load per wave and round).  Inside a round the lanes
// that keep their element are ranked by a ballot; the rounds of a wave follow each other, the waves' totals meet in LDS.  The
// kept elements are staged in LDS at their rank in the tile and leave from there, keys and values as two coalesced streams.
#pragma once
#include "pdl_common.h"
#include "pdl_scan.h"

constexpr uint32_t RM_GONE = 0xffffffffu;
constexpr int RM_THREADS = 256, RM_ITEMS = 8, RM_WAVES = RM_THREADS / PDL_WAVE;
constexpr int RM_WAVE_SPAN = RM_ITEMS * PDL_WAVE, RM_TILE = RM_THREADS * RM_ITEMS;

// ---- R-map ------------------------------------------------------------------------------------------------------------------
struct RmStays {
    const uint32_t *gen, *gmap;
    __device__ uint32_t operator()(uint64_t i) const { return gmap[gen[i]] != RM_GONE ? 1u : 0u; }
};
struct RmMapApply {
    const uint32_t *gen, *gmap, *kseq, *glen;
    uint32_t *new_id, *out_gen, *out_kseq, *out_glen;
    unsigned long long *gone_residues;
    __device__ void operator()(uint64_t i, uint32_t stays, uint32_t prefix) const {
        if (stays) {
            new_id[i] = prefix;
            out_gen[prefix] = gmap[gen[i]]; out_kseq[prefix] = kseq[i]; out_glen[prefix] = glen[i];
        } else {
            new_id[i] = RM_GONE;
            atomicAdd(gone_residues, (unsigned long long) glen[i]);        // (the genes of r genomes out of G: a few hundred adds)
        }
    }
};

// ---- R-compact + R-alpha ----------------------------------------------------------------------------------------------------
// x / base for a 32-bit x by one multiplication: magic = ceil(2^64 / base) (Lemire, Kaser & Kurz 2019: exact for every x < 2^32)
struct RmDigits {
    uint32_t k, base;
    uint64_t magic;
};
inline RmDigits rm_digits(uint32_t k, uint32_t base) { return RmDigits{k, base, base > 1 ? ~0ull / base + 1 : 0ull}; }

// the wave's slice of the tile: element (round j, lane) is at slice + j * 64
__device__ __forceinline__ uint64_t rm_slice(uint32_t wave, uint32_t lane) {
    return (uint64_t) blockIdx.x * RM_TILE + (uint64_t) wave * RM_WAVE_SPAN + lane;
}

__global__ __launch_bounds__(RM_THREADS) void k_rm_count(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ new_id, uint64_t m,
                                                         uint32_t *__restrict__ tile_sums) {
    __shared__ uint32_t s_wave[RM_WAVES];
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1), wave = threadIdx.x / PDL_WAVE;
    const uint64_t at = rm_slice(wave, lane);
    uint32_t v[RM_ITEMS];
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {             // (index clamped, result masked: the loads of all rounds overlap)
        const uint64_t i = at + (uint64_t) j * PDL_WAVE;
        v[j] = vals[i < m ? i : m - 1];
    }
    uint32_t kept = 0;
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {
        const uint64_t i = at + (uint64_t) j * PDL_WAVE;
        kept += (uint32_t) __popcll(__ballot(i < m && new_id[v[j]] != RM_GONE));
    }
    if (lane == 0) s_wave[wave] = kept;
    pdl_sync();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < RM_WAVES; w++) total += s_wave[w];
        tile_sums[blockIdx.x] = total;
    }
}

// tile_off: the exclusive scan of k_rm_count's sums.  seen[d] = 1 for every base-B digit d of a key that stays.
template <class KeyT>
__global__ __launch_bounds__(RM_THREADS) void k_rm_compact(const KeyT *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                           const uint32_t *__restrict__ new_id, uint64_t m, const uint32_t *__restrict__ tile_off,
                                                           KeyT *__restrict__ out_keys, uint32_t *__restrict__ out_vals, RmDigits dg,
                                                           uint32_t *__restrict__ seen) {
    __shared__ KeyT s_key[RM_TILE];
    __shared__ uint32_t s_val[RM_TILE];
    __shared__ uint32_t s_wave[RM_WAVES];
    __shared__ uint32_t s_seen[256];
    const uint32_t tid = threadIdx.x, lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
    s_seen[tid] = 0;
    const uint64_t at = rm_slice(wave, lane);
    KeyT key[RM_ITEMS];
    uint32_t id[RM_ITEMS];
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {
        const uint64_t i = at + (uint64_t) j * PDL_WAVE;
        const uint64_t ic = i < m ? i : m - 1;
        key[j] = keys[ic]; id[j] = vals[ic];
    }
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {
        const uint64_t i = at + (uint64_t) j * PDL_WAVE;
        id[j] = i < m ? new_id[id[j]] : RM_GONE;    // (the one gather per element; a leaving gene and a slot past the end look alike)
    }
    // rank of every kept element inside the wave's slice: lanes of a round by ballot, rounds one after the other
    uint32_t pos[RM_ITEMS];
    uint32_t run = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {
        const unsigned long long b = __ballot(id[j] != RM_GONE);
        pos[j] = run + (uint32_t) __popcll(b & below);
        run += (uint32_t) __popcll(b);
    }
    if (lane == 0) s_wave[wave] = run;
    pdl_sync();                                      // (s_seen is cleared, the waves' totals are in place)
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RM_WAVES; w++) {
        const uint32_t t = s_wave[w];
        base += (uint32_t) w < wave ? t : 0u;
        total += t;
    }
#pragma unroll
    for (int j = 0; j < RM_ITEMS; j++) {
        if (id[j] == RM_GONE) continue;
        s_key[base + pos[j]] = key[j]; s_val[base + pos[j]] = id[j];
        // R-alpha: the k digits of the key name letters the remaining set certainly holds.  Lanes that meet the same digit store
        // the same value to the same word (no atomic, as in K-hist).
        KeyT x = key[j];
        for (uint32_t d = 0; d < dg.k; d++) {
            KeyT q;
            if constexpr (sizeof(KeyT) == 4) q = (KeyT) __umul64hi((uint64_t) x, dg.magic);
            else q = x / dg.base;
            s_seen[(uint32_t) (x - q * dg.base) & 255u] = 1u;
            x = q;
        }
    }
    pdl_sync();
    const uint64_t out0 = tile_off[blockIdx.x];
    for (uint32_t e = tid; e < total; e += RM_THREADS) { out_keys[out0 + e] = s_key[e]; out_vals[out0 + e] = s_val[e]; }
    if (s_seen[tid]) seen[tid] = 1u;
}

// (out_keys, out_vals)[0 .. m') = the elements of (keys, vals)[0 .. m) whose gene stays, in their order, values renumbered;
// m' -> *d_kept.  `tile` holds pdl_remove_tiles(m) words; out_keys / out_vals hold m elements; m >= 1.
inline size_t pdl_remove_tiles(uint64_t m) { return (size_t) ((m + RM_TILE - 1) / RM_TILE); }
template <class KeyT>
static void pdl_compact_stream(hipStream_t st, const KeyT *keys, const uint32_t *vals, const uint32_t *new_id, uint64_t m, uint32_t *tile,
                               KeyT *out_keys, uint32_t *out_vals, RmDigits dg, uint32_t *seen, uint64_t *d_kept) {
    const uint32_t tiles = (uint32_t) pdl_remove_tiles(m);
    hipLaunchKernelGGL(k_rm_count, dim3(tiles), dim3(RM_THREADS), 0, st, vals, new_id, m, tile);
    hipLaunchKernelGGL(k_scan_tile_scan, dim3(1), dim3(1024), 0, st, tile, tiles, d_kept, (uint64_t *) nullptr);
    hipLaunchKernelGGL(k_rm_compact<KeyT>, dim3(tiles), dim3(RM_THREADS), 0, st, keys, vals, new_id, m, (const uint32_t *) tile, out_keys, out_vals, dg, seen);
    PDL_HIP(hipGetLastError());
}
