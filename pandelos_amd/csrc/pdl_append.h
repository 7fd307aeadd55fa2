// pdl_append.h — K-merge: the sorted k-mer stream of a context grows by the sorted stream of appended genes
// (pdl_append_genomes, include/pandelos_amd.h), included from pdl_dict.hip, whose stages the append runs around it.
//
// The union's stream is what the stable LSD sort by rank (pdl_sort_pairs, library.cpp:172-187,270-278) would leave for
// base genes + new genes: both inputs are in that order already, every new gene id is above every base id, so the union
// is their STABLE MERGE with the base element first on equal keys.  "Key" is the part of the rank the sort covers: all
// of it normally; where ranks wrapped past 2^64 unnoticed (RankParams::key_bits != rank_bits) the sort's passes stop
// at the last byte rank_bits reaches and the stream is ordered by those low bytes only — `mask` selects them.
//
//   k_merge_partition   one thread per tile boundary: the diagonal binary search (merge path) over (base, new);
//                       split[t] = base elements among the first t * MG_TILE outputs
//   k_merge_tiles       one workgroup per tile of MG_TILE outputs.  A tile without a new element is a copy, sixteen bytes
//                       per lane, no LDS.  Otherwise both slices are staged in LDS, every thread finds the sub-diagonal
//                       of its MG_ITEMS outputs, merges them in registers, and the tile leaves through LDS, coalesced.
//
// LDS layout: element i of the tile lives at i + i / 32.  The threads of a wave walk slices that start MG_ITEMS = 8
// elements apart: unpadded, 32 lanes fall on 4 banks (4-byte keys; 8-byte keys: 16 dwords apart on the 64-bank read) —
// eight addresses per bank; with one element of padding per 32 the 32 lanes of a group fall on 32 different banks, and so
// do the four consecutive elements a lane stages from one 16-byte load.
#pragma once
#include "pdl_common.h"

constexpr int MG_THREADS = 256, MG_ITEMS = 8, MG_TILE = MG_THREADS * MG_ITEMS;
constexpr int MG_LDS = MG_TILE + MG_TILE / 32;

__device__ __forceinline__ uint32_t mg_pad(uint32_t i) { return i + (i >> 5); }

// base elements among the first `diag` outputs: the smallest a with NOT (base[a] <= new[diag - 1 - a])
template <class KeyT, class GetA, class GetB>
__device__ __forceinline__ uint32_t mg_diagonal(uint32_t diag, uint32_t na, uint32_t nb, KeyT mask, GetA key_a, GetB key_b) {
    uint32_t lo = diag > nb ? diag - nb : 0u, hi = diag < na ? diag : na;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((key_a(mid) & mask) <= (key_b(diag - 1 - mid) & mask)) lo = mid + 1; else hi = mid;     // a tie: the base element goes first
    }
    return lo;
}

template <class KeyT>
__global__ __launch_bounds__(256) void k_merge_partition(const KeyT *__restrict__ a_keys, uint32_t na, const KeyT *__restrict__ b_keys, uint32_t nb,
                                                         KeyT mask, uint32_t tiles, uint32_t *__restrict__ split) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t > tiles) return;
    const uint64_t d64 = (uint64_t) t * MG_TILE;
    const uint32_t diag = (uint32_t) (d64 < (uint64_t) na + nb ? d64 : (uint64_t) na + nb);
    split[t] = mg_diagonal<KeyT>(diag, na, nb, mask, [&](uint32_t i) { return a_keys[i]; }, [&](uint32_t i) { return b_keys[i]; });
}

// sixteen bytes of keys / values from an address that is only element-aligned (a tile's slice starts anywhere)
template <class T> struct __attribute__((packed, aligned(sizeof(T)))) MgVec { T v[16 / sizeof(T)]; };

// dst[0 .. n) = src[0 .. n): 16-byte loads (element-aligned) and 16-byte stores (dst is 16-byte aligned: a tile's first output)
template <class T>
__device__ __forceinline__ void mg_copy(T *__restrict__ dst, const T *__restrict__ src, uint32_t n) {
    constexpr uint32_t E = 16 / sizeof(T);
    const uint32_t chunks = n / E;
    for (uint32_t ch = threadIdx.x; ch < chunks; ch += MG_THREADS) {
        const MgVec<T> v = *reinterpret_cast<const MgVec<T> *>(src + ch * E);
        uint4 w;
        __builtin_memcpy(&w, &v, 16);
        *reinterpret_cast<uint4 *>(dst + ch * E) = w;
    }
    for (uint32_t i = chunks * E + threadIdx.x; i < n; i += MG_THREADS) dst[i] = src[i];
}

// s[pad(at + i)] = src[i] + add for i in [0, n): 16-byte loads, one LDS store per element
template <class T>
__device__ __forceinline__ void mg_stage(T *s, uint32_t at, const T *__restrict__ src, uint32_t n, T add) {
    constexpr uint32_t E = 16 / sizeof(T);
    const uint32_t chunks = n / E;
    for (uint32_t ch = threadIdx.x; ch < chunks; ch += MG_THREADS) {
        const MgVec<T> v = *reinterpret_cast<const MgVec<T> *>(src + ch * E);
#pragma unroll
        for (uint32_t j = 0; j < E; j++) s[mg_pad(at + ch * E + j)] = v.v[j] + add;
    }
    for (uint32_t i = chunks * E + threadIdx.x; i < n; i += MG_THREADS) s[mg_pad(at + i)] = src[i] + add;
}

template <class KeyT>
__global__ __launch_bounds__(MG_THREADS) void k_merge_tiles(const KeyT *__restrict__ a_keys, const uint32_t *__restrict__ a_vals, uint32_t na,
                                                           const KeyT *__restrict__ b_keys, const uint32_t *__restrict__ b_vals, uint32_t nb,
                                                           uint32_t b_val_add, KeyT mask, const uint32_t *__restrict__ split,
                                                           KeyT *__restrict__ out_keys, uint32_t *__restrict__ out_vals) {
    __shared__ KeyT s_key[MG_LDS];
    __shared__ uint32_t s_val[MG_LDS];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = na + nb;
    const uint32_t d0 = tile * MG_TILE, d1 = min(d0 + (uint32_t) MG_TILE, total);
    const uint32_t a0 = split[tile], a1 = split[tile + 1];
    const uint32_t b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t ta = a1 - a0, tb = b1 - b0, cnt = d1 - d0;       // this tile: ta base elements, tb new ones
    if (tb == 0) {                                                  // (uniform) nothing new under this tile: the base slice as it is
        mg_copy<KeyT>(out_keys + d0, a_keys + a0, ta);
        mg_copy<uint32_t>(out_vals + d0, a_vals + a0, ta);
        return;
    }
    // the tile's inputs: base slice at [0, ta), new slice at [ta, cnt); the new genes' ids are made here
    mg_stage<KeyT>(s_key, 0, a_keys + a0, ta, (KeyT) 0);
    mg_stage<uint32_t>(s_val, 0, a_vals + a0, ta, 0u);
    mg_stage<KeyT>(s_key, ta, b_keys + b0, tb, (KeyT) 0);
    mg_stage<uint32_t>(s_val, ta, b_vals + b0, tb, b_val_add);
    pdl_sync();
    // the thread's MG_ITEMS outputs start at diagonal tid * MG_ITEMS of the tile
    const uint32_t diag = min(tid * MG_ITEMS, cnt);
    auto key_at = [&](uint32_t i) { return s_key[mg_pad(i < (uint32_t) MG_TILE ? i : (uint32_t) MG_TILE - 1)]; };      // (in bounds whatever i: exhausted slices read a slot nobody uses)
    uint32_t ai = mg_diagonal<KeyT>(diag, ta, tb, mask, [&](uint32_t i) { return key_at(i); }, [&](uint32_t i) { return key_at(ta + i); });
    uint32_t bi = diag - ai;
    KeyT ka = key_at(ai), kb = key_at(ta + bi);
    KeyT ok[MG_ITEMS];
    uint32_t src[MG_ITEMS];
#pragma unroll
    for (int j = 0; j < MG_ITEMS; j++) {
        const bool take_a = bi >= tb || (ai < ta && (ka & mask) <= (kb & mask));
        ok[j] = take_a ? ka : kb;
        src[j] = take_a ? ai : ta + bi;
        if (take_a) { ai++; ka = key_at(ai); } else { bi++; kb = key_at(ta + bi); }
    }
    uint32_t ov[MG_ITEMS];
#pragma unroll
    for (int j = 0; j < MG_ITEMS; j++) ov[j] = s_val[mg_pad(src[j] < (uint32_t) MG_TILE ? src[j] : (uint32_t) MG_TILE - 1)];
    pdl_sync();                                                     // every thread has read its inputs: the tile's output takes their place
#pragma unroll
    for (int j = 0; j < MG_ITEMS; j++) {
        const uint32_t e = tid * MG_ITEMS + j;
        s_key[mg_pad(e)] = ok[j]; s_val[mg_pad(e)] = ov[j];
    }
    pdl_sync();
#pragma unroll
    for (int j = 0; j < MG_ITEMS; j++) {
        const uint32_t e = j * MG_THREADS + tid;                    // coalesced, keys and gene values as two streams
        if (e < cnt) { out_keys[d0 + e] = s_key[mg_pad(e)]; out_vals[d0 + e] = s_val[mg_pad(e)]; }
    }
}

// (out_keys, out_vals)[0 .. na + nb) = stable merge of (a, na) and (b, nb) on key & mask, a first on ties; b's values + b_val_add.
// `split` holds (na + nb) / MG_TILE + 2 words.  na + nb < 2^32 (checked by the caller).
template <class KeyT>
static void pdl_merge_streams(hipStream_t st, const KeyT *a_keys, const uint32_t *a_vals, uint32_t na, const KeyT *b_keys, const uint32_t *b_vals,
                              uint32_t nb, uint32_t b_val_add, KeyT mask, uint32_t *split, KeyT *out_keys, uint32_t *out_vals) {
    const uint32_t tiles = (uint32_t) (((uint64_t) na + nb + MG_TILE - 1) / MG_TILE);
    if (!tiles) return;
    hipLaunchKernelGGL(k_merge_partition<KeyT>, dim3((tiles + 1 + 255) / 256), dim3(256), 0, st, a_keys, na, b_keys, nb, mask, tiles, split);
    hipLaunchKernelGGL(k_merge_tiles<KeyT>, dim3(tiles), dim3(MG_THREADS), 0, st, a_keys, a_vals, na, b_keys, b_vals, nb, b_val_add, mask,
                       (const uint32_t *) split, out_keys, out_vals);
    PDL_HIP(hipGetLastError());
}
inline size_t pdl_merge_split_words(uint64_t total) { return (size_t) ((total + MG_TILE - 1) / MG_TILE) + 2; }
