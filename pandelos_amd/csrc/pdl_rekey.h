// pdl_rekey.h — K-rekey: the sorted k-mer stream of a context is written again for another alphabet (option "alphabet_rekey" of
// pdl_append_genomes / pdl_remove_genomes, include/pandelos_amd.h), included from pdl_dict.hip.
//
// A polynomial rank with an exact B^k is its k-mer written in base B with the dense digits rank_values[letter] (library.cpp:
// 75-86, 96-99).  When letters join or leave the alphabet, B becomes B' and every digit d becomes map[d], and map is strictly
// increasing on the letters both alphabets hold: digit by digit the order of two k-mers stays what it was, so
//     key' = sum map[d_i] * B'^i        (d_i: digit i of the key in base B, low digit first)
// is monotone in the key and equal keys stay equal.  The stream (keys, vals) stays sorted by (rank, input position): one
// streaming pass over the keys leaves what the sort of the new set's build would have left; the values are not touched.
//
//   decode   a key below 2^32 gives its digits by one multiplication each (RmDigits of pdl_remove.h: magic = ceil(2^64 / B),
//            exact for every x < 2^32).  A 64-bit key is first cut into parts of h digits, h the most with B^h <= 2^32, by a
//            multiply-high with floor(2^64 / B^h) and one correction (the estimate is the quotient or one below it); since
//            B^(h+1) > 2^32 and B^k < 2^64, k <= 2h + 1: three parts at most, the third a single digit.
//   map +    one table T[i][d] = map[d] * B'^i of k * B entries (at most 2040 where B^k < 2^64: 16 KB), made by the host, in LDS:
//   encode   key' = sum T[i][d_i] — an LDS load and an add per digit instead of a byte load and a 64-bit multiplication.
//
// A thread takes four consecutive keys (16-byte loads and stores; the streams start at allocations), its four digit chains
// side by side; the m % 4 keys of the tail go one to a thread of the first workgroup.
//
// Q-rebase (option "query_rekey" of the query entry points, pdl_query.h) uses the same plan the other way round for single keys: a
// query ranked in a superset alphabet has its records' keys written back into the base's (rk_one, k_q_rebase), see there; what it
// leaves (QRebased) is the `r` of the views QView / QBView<KeyB, KeyQ, true> that k_q_fold, k_q_match, k_qb_fold and k_qb_match read.
//
// The host section is what an append and a removal share before the context changes (tools/rekey_host_check.cpp runs it without a
// device): rank_init_host (the build's too), rk_exact, rk_plan, rk_change — the one decision: the same letters, a re-key, or a
// target that is not exact — and the short_letters_* functions that keep pdl_ctx::h_short_letters.
#pragma once
#include "pdl_common.h"
#include "pdl_remove.h"

#include <cstring>

constexpr int RK_THREADS = 256, RK_ITEMS = 4;     // (RkArgs, the kernels' arguments: pdl_common.h)

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The rank table of an alphabet: library.cpp:88-132, literally (64-bit wraparound included); adds rank_bits for the device sort and
// key_bits.  The build (stage_alphabet_and_lengths, pdl_dict.hip) and rk_change below make every table of a context through it.
inline void rank_init_host(RankParams &rp, const uint64_t counters[256], int kvalue) {
    memset(&rp, 0, sizeof(rp));
    rp.k = (uint32_t) kvalue;
    int rank = 0;
    for (int i = 0; i < 256; i++)
        if (counters[i] > 0) rp.rank_values[i] = (uint8_t) rank++;
    const uint8_t rank_base = (uint8_t) rank;
    rp.base = rank_base;
    uint64_t last_multiplier = 1;
    bool has_overflow = false;
    int tmp_kvalue = kvalue - 1;
    while (tmp_kvalue--) {
        uint64_t ovflw_test = last_multiplier;
        last_multiplier *= rank_base;
        if (has_overflow) {
            last_multiplier %= RABIN_MODULO;
        } else if ((ovflw_test > last_multiplier) || (ovflw_test * rank_base > last_multiplier * rank_base)) {
            has_overflow = true;
            last_multiplier = ((ovflw_test % RABIN_MODULO) * rank_base) % RABIN_MODULO;
        }
    }
    rp.last_multiplier = last_multiplier;
    rp.hash_fallback = has_overflow ? 1u : 0u;
    rp.key_bits = 64;
    if (has_overflow) {
        rp.rank_bits = 64;
    } else {
        uint64_t rank_tmp = last_multiplier * rank_base;   // B^k, fits (the loop above looked one step ahead)
        rp.rank_bits = rank_tmp ? bit_length64(rank_tmp - 1) : 1;
        if (rp.rank_bits == 0) rp.rank_bits = 1;
        if (pow_fits_u64(rank_base, (uint32_t) kvalue)) rp.key_bits = rp.rank_bits;      // did B^k fit?
    }
}

// ranks are the polynomial itself, so a key decodes into letters: no hashing, and B^k fits 64 bits EXACTLY (pow_fits_u64)
inline bool rk_exact(const RankParams &rp) { return !rp.hash_fallback && rp.base != 0 && pow_fits_u64(rp.base, rp.k); }
inline const char *rk_why_not(const RankParams &rp) { return rp.hash_fallback ? "hashed" : "wrapped past 2^64"; }

// The plan of a re-key from (from, present_from) to (to, present_to), both exact, same k: the kernel's arguments and the table
// (as 64-bit words; the launch narrows them for 32-bit output).  A letter only `from` holds has no image: its row entries stay
// 0, and no key that is re-keyed holds it (a removal re-keys what stays).
inline RkArgs rk_plan(const RankParams &from, const uint8_t present_from[256], const RankParams &to, const uint8_t present_to[256],
                      std::vector<uint64_t> &table) {
    RkArgs a{};
    a.k = from.k; a.base = from.base;
    a.magic = rm_digits(from.k, from.base).magic;
    a.h = 0; a.part_div = 1;
    while (a.h < a.k && a.part_div * from.base <= (1ull << 32)) { a.part_div *= from.base; a.h++; }      // (B <= 256: h >= 1)
    a.nparts = (a.k + a.h - 1) / a.h;
    a.part_magic = a.part_div > 1 ? ~0ull / a.part_div + (~0ull % a.part_div == a.part_div - 1 ? 1 : 0) : 0;
    a.entries = a.k * a.base;
    table.assign(a.entries, 0);
    uint64_t pw = 1;
    for (uint32_t i = 0; i < a.k; i++) {
        for (int b = 0; b < 256; b++)
            if (present_from[b] && present_to[b]) table[(size_t) i * a.base + from.rank_values[b]] = (uint64_t) to.rank_values[b] * pw;
        pw *= to.base;          // (B'^k fits: the last product is not used beyond it)
    }
    return a;
}

// What a call that changes the set decides about the alphabet before the context changes: the letters afterwards, their rank
// table as a build makes it and, when the letters differ (rekey), the plan that writes the stream's keys again.
struct RkChange { bool rekey = false; RankParams rp{}; uint8_t present[256] = {}; RkArgs args{}; };
// (from, present_from), exact, becomes the alphabet present_to: equal letters leave ch.rekey false; else ch.rp is
// rank_init_host of them and, when it is exact too, ch.args / table the plan.  false: the target is not exact (ch.rp says why,
// rk_why_not) and nothing can be re-keyed — the refusal and its words are the caller's.
inline bool rk_change(const RankParams &from, const uint8_t present_from[256], const uint8_t present_to[256], std::vector<uint64_t> &table,
                      RkChange &ch) {
    ch = RkChange{};
    uint64_t counters[256];
    bool same = true;
    for (int b = 0; b < 256; b++) { counters[b] = ch.present[b] = present_to[b] ? 1 : 0; same = same && ch.present[b] == (present_from[b] ? 1 : 0); }
    if (same) { ch.rp = from; return true; }
    rank_init_host(ch.rp, counters, (int) from.k);
    if (!rk_exact(ch.rp)) return false;
    ch.args = rk_plan(from, present_from, ch.rp, ch.present, table);
    return ch.rekey = true;
}

// What queries that bring `letters` (256 bits, bytes the base lacks among them or not) decide about the alphabet they are ranked
// in (option "query_rekey"): the base's letters plus theirs.  (base, present_base) is exact.  false: that union is not exact
// (q.up.rp says why).  Else q.up is the change base -> union (q.up.rekey false: no new letter at all) with its forward table,
// q.down / q.down_table the plan union -> base that Q-rebase reads — a new letter's entries are 0 there — and q.absent the
// union's digits that are new letters.
struct RkQuery { RkChange up; std::vector<uint64_t> up_table, down_table; RkArgs down{}; uint32_t absent[8] = {}; };
inline bool rk_query(const RankParams &base, const uint8_t present_base[256], const uint32_t letters[8], RkQuery &q) {
    uint8_t present_to[256];
    for (int b = 0; b < 256; b++) present_to[b] = (present_base[b] || ((letters[b >> 5] >> (b & 31)) & 1u)) ? 1 : 0;
    memset(q.absent, 0, sizeof(q.absent));
    if (!rk_change(base, present_base, present_to, q.up_table, q.up)) return false;
    if (!q.up.rekey) return true;
    q.down = rk_plan(q.up.rp, q.up.present, base, present_base, q.down_table);
    for (int b = 0; b < 256; b++)
        if (present_to[b] && !present_base[b]) { const uint32_t d = q.up.rp.rank_values[b]; q.absent[d >> 5] |= 1u << (d & 31); }
    return true;
}

// ---- the letters of genes shorter than k, per genome (256 bits each, pdl_ctx::h_short_letters): they show in no key, and a removal
// must know them.  Filled behind a build (k_short_letters below), then kept up on the host by every append and removal.
// behind a build: the device's table becomes the context's own, a few words a genome (the stream has been waited for)
inline void short_letters_fetch(std::vector<uint32_t> &h, const void *d_letters, uint32_t n_genomes) {
    h.assign((size_t) n_genomes * 8, 0u);
    PDL_HIP(hipMemcpy(h.data(), d_letters, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
}
// an append: the letters of the new genomes' genes shorter than k (a handful of residues: on the host); n_genomes counts the new ones in
inline void short_letters_append(std::vector<uint32_t> &h, uint32_t n_genomes, const uint8_t *residues, const uint64_t *offsets,
                                 const uint32_t *genome_ids, uint32_t n, uint32_t k) {
    h.resize((size_t) n_genomes * 8, 0u);
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] - offsets[i] < k)
            for (uint64_t r = offsets[i]; r < offsets[i + 1]; r++) h[(size_t) genome_ids[i] * 8 + (residues[r] >> 5)] |= 1u << (residues[r] & 31);
}
// a removal, before it decides: is[b] = a gene shorter than k of a genome that stays (gmap[g] != RM_GONE) holds the byte b
inline void short_letters_staying(const std::vector<uint32_t> &h, const std::vector<uint32_t> &gmap, uint8_t is[256]) {
    uint32_t bits[8] = {};
    for (size_t g = 0; g < gmap.size(); g++) for (size_t w = 0; w < 8 && gmap[g] != RM_GONE; w++) bits[w] |= h[g * 8 + w];
    for (int b = 0; b < 256; b++) is[b] = (uint8_t) (bits[b >> 5] >> (b & 31) & 1u);
}
// a removal, once it goes through: the table closes up like the genome ids (gmap ascends over the genomes that stay)
inline void short_letters_remove(std::vector<uint32_t> &h, const std::vector<uint32_t> &gmap, uint32_t n_genomes_left) {
    for (size_t g = 0; g < gmap.size(); g++)
        if (gmap[g] != RM_GONE && gmap[g] != g) memcpy(&h[(size_t) gmap[g] * 8], &h[g * 8], 32);
    h.resize((size_t) n_genomes_left * 8);
}

#ifdef __HIPCC__
// ---- device --------------------------------------------------------------------------------------------------------------------
template <class KeyIn, class KeyOut>
__device__ __forceinline__ void rk_items(const KeyIn (&x)[RK_ITEMS], KeyOut (&y)[RK_ITEMS], const RkArgs &a, const KeyOut *T) {
    uint64_t rest[RK_ITEMS];
#pragma unroll
    for (int j = 0; j < RK_ITEMS; j++) { rest[j] = x[j]; y[j] = 0; }
    uint32_t left = a.k, row = 0;
    for (uint32_t p = 0; p < a.nparts; p++) {                       // (uniform: one part for 32-bit keys, three at most)
        const uint32_t nd = left < a.h ? left : a.h;
        uint32_t part[RK_ITEMS];
#pragma unroll
        for (int j = 0; j < RK_ITEMS; j++) {
            if (sizeof(KeyIn) == 8 && p + 1 < a.nparts) {
                uint64_t q = __umul64hi(rest[j], a.part_magic);     // the quotient or one below it
                uint64_t r = rest[j] - q * a.part_div;
                if (r >= a.part_div) { q++; r -= a.part_div; }
                part[j] = (uint32_t) r; rest[j] = q;
            } else part[j] = (uint32_t) rest[j];                    // (the last part is below B^h <= 2^32)
        }
        for (uint32_t i = 0; i < nd; i++, row += a.base) {
#pragma unroll
            for (int j = 0; j < RK_ITEMS; j++) {
                const uint32_t q = (uint32_t) __umul64hi((uint64_t) part[j], a.magic);
                const uint32_t d = part[j] - q * a.base;            // (< base: row + d < entries)
                y[j] += T[row + d];
                part[j] = q;
            }
        }
        left -= nd;
    }
}

template <class KeyIn, class KeyOut>
__global__ __launch_bounds__(RK_THREADS) void k_rekey(const KeyIn *__restrict__ in, KeyOut *__restrict__ out, uint64_t m, RkArgs a,
                                                      const KeyOut *__restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rk_lds[];
    KeyOut *T = reinterpret_cast<KeyOut *>(rk_lds);
    for (uint32_t i = threadIdx.x; i < a.entries; i += RK_THREADS) T[i] = table[i];
    pdl_sync();
    constexpr int WI = sizeof(KeyIn) * RK_ITEMS / 16, WO = sizeof(KeyOut) * RK_ITEMS / 16;
    const uint4 *in16 = reinterpret_cast<const uint4 *>(in);
    uint4 *out16 = reinterpret_cast<uint4 *>(out);
    const uint64_t chunks = m / RK_ITEMS, stride = (uint64_t) gridDim.x * RK_THREADS;
    KeyIn x[RK_ITEMS];
    KeyOut y[RK_ITEMS];
    for (uint64_t ch = (uint64_t) blockIdx.x * RK_THREADS + threadIdx.x; ch < chunks; ch += stride) {
        uint4 w[WI];
#pragma unroll
        for (int i = 0; i < WI; i++) w[i] = in16[ch * WI + i];
        __builtin_memcpy(x, w, sizeof(x));
        rk_items<KeyIn, KeyOut>(x, y, a, T);
        uint4 v[WO];
        __builtin_memcpy(v, y, sizeof(y));
#pragma unroll
        for (int i = 0; i < WO; i++) out16[ch * WO + i] = v[i];
    }
    const uint64_t t = chunks * RK_ITEMS + threadIdx.x;            // the tail: a key a thread
    if (blockIdx.x == 0 && t < m) {
#pragma unroll
        for (int j = 0; j < RK_ITEMS; j++) x[j] = in[t];
        rk_items<KeyIn, KeyOut>(x, y, a, T);
        out[t] = y[0];
    }
}

// out[0 .. m) = in[0 .. m) re-keyed by (a, table); `in` and `out` are 16-byte aligned and distinct; `d_table` holds a.entries KeyOut words
template <class KeyIn, class KeyOut>
static void pdl_rekey_stream(hipStream_t st, const KeyIn *in, KeyOut *out, uint64_t m, const RkArgs &a, const KeyOut *d_table) {
    if (!m) return;
    const uint64_t blocks = (m / RK_ITEMS + RK_THREADS - 1) / RK_THREADS;
    hipLaunchKernelGGL((k_rekey<KeyIn, KeyOut>), dim3((uint32_t) std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 4096)), dim3(RK_THREADS),
                       (size_t) a.entries * sizeof(KeyOut), st, in, out, m, a, d_table);
    PDL_HIP(hipGetLastError());
}

// ---- Q-rebase (option "query_rekey", pdl_query.h) ------------------------------------------------------------------------------
// A query that brings letters the base lacks is ranked in the union's alphabet (B' letters); its records search the base's keys,
// which stay in the base's (B letters).  The digit map base -> union is strictly increasing, so its inverse on the digits that
// have one keeps order and equality: a query key written back digit by digit, key_b = sum inv[d_i] * B^i, compares with a base
// key exactly as the two k-mers compare in the union — and a key with a digit that has no inverse (a new letter) equals no
// base key at all.  That is said by a flag beside the key, not by a key value.
//
// One key taken apart as rk_items takes four: parts of h digits, a multiplication per digit, a table load and an add.
// T[row + d] with row = i * base and d < base (a remainder), i < k: below entries = k * base whatever the key is.
// `absent`: 256 bits over the digits, or null; hit = some digit of the key has its bit set.
template <class KeyOut>
__device__ __forceinline__ KeyOut rk_one(uint64_t x, const RkArgs &a, const KeyOut *T, const uint32_t *absent, bool &hit) {
    uint64_t rest = x;
    KeyOut y = 0;
    uint32_t left = a.k, row = 0, seen = 0;
    for (uint32_t p = 0; p < a.nparts; p++) {                       // (uniform: three parts at most)
        const uint32_t nd = left < a.h ? left : a.h;
        uint32_t part;
        if (p + 1 < a.nparts) {
            uint64_t q = __umul64hi(rest, a.part_magic);            // the quotient or one below it
            uint64_t r = rest - q * a.part_div;
            if (r >= a.part_div) { q++; r -= a.part_div; }
            part = (uint32_t) r; rest = q;
        } else part = (uint32_t) rest;                              // (the last part is below B^h <= 2^32)
        for (uint32_t i = 0; i < nd; i++, row += a.base) {
            const uint32_t q = (uint32_t) __umul64hi((uint64_t) part, a.magic);
            const uint32_t d = part - q * a.base;                   // (< base: row + d < entries, d < 256)
            y += T[row + d];
            if (absent) seen |= (absent[d >> 5] >> (d & 31)) & 1u;
            part = q;
        }
        left -= nd;
    }
    hit = seen != 0;
    return y;
}

// The three ranks the fold reads from the base's keys (q_fold_base, pdl_query.h: bmax and the ranks of the last two records),
// in the union's alphabet: up3[0 .. 3).  One thread, the forward table (rk_plan base -> union, 64-bit words) in global memory.
// U >= 1 and M >= 1: the context is built.
template <class KeyB>
__global__ void k_q_up3(const KeyB *__restrict__ bkeys, const uint32_t *__restrict__ brecpos, uint32_t U, uint64_t M, RkArgs a,
                        const uint64_t *__restrict__ table, unsigned long long *__restrict__ up3) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool hit;
    up3[0] = rk_one<uint64_t>(bkeys[M - 1], a, table, nullptr, hit);
    up3[1] = rk_one<uint64_t>(bkeys[brecpos[U - 1]], a, table, nullptr, hit);
    up3[2] = U >= 2 ? rk_one<uint64_t>(bkeys[brecpos[U - 2]], a, table, nullptr, hit) : 0ull;
}

// Q-rebase: query record j (j below the record count on the device and below the host's bound, as k_q_match) has the union key
// qkeys[recpos[j]] (recpos null: qkeys[j]); bkey[j] = that key in the base's alphabet, none[j] = 1 when it holds a new letter.
// `a` / `table`: rk_plan union -> base (a new letter's entries are 0), the table in LDS; absent: the union's digits that are
// new letters.  One thread a record: a query holds 1 / (G + 1) of the records.
struct RkAbsent { uint32_t bits[8]; };
template <class KeyQ, class KeyB>
__global__ __launch_bounds__(RK_THREADS) void k_q_rebase(const KeyQ *__restrict__ qkeys, const uint32_t *__restrict__ recpos,
                                                         const unsigned long long *__restrict__ d_records, uint64_t bound, RkArgs a,
                                                         const KeyB *__restrict__ table, RkAbsent ab, KeyB *__restrict__ bkey,
                                                         uint8_t *__restrict__ none) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rb_lds[];
    __shared__ uint32_t s_absent[8];
    KeyB *T = reinterpret_cast<KeyB *>(rb_lds);
    for (uint32_t i = threadIdx.x; i < a.entries; i += RK_THREADS) T[i] = table[i];
    if (threadIdx.x < 8) s_absent[threadIdx.x] = ab.bits[threadIdx.x];
    pdl_sync();
    const uint64_t records = *d_records, n = records < bound ? records : bound;
    const uint64_t j = (uint64_t) blockIdx.x * RK_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t x = (uint64_t) (recpos ? qkeys[recpos[j]] : qkeys[j]);
    bool hit;
    bkey[j] = rk_one<KeyB>(x, a, T, s_absent, hit);
    none[j] = hit ? 1 : 0;
}

// ---- the letters of genes shorter than k, per genome (256 bits each): they show in no key, and a removal must know them -----------
__global__ __launch_bounds__(256) void k_short_letters(const uint8_t *__restrict__ res, const uint64_t *__restrict__ off, const uint32_t *__restrict__ gen,
                                                       uint32_t n, uint32_t n_genomes, uint32_t k, uint64_t n_res, uint32_t *__restrict__ letters) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = off[i], e = off[i + 1];
    if (e <= b || e - b >= k || e > n_res) return;
    const uint32_t g = gen[i];
    if (g >= n_genomes) return;
    for (uint64_t r = b; r < e; r++) atomicOr(&letters[(size_t) g * 8 + (res[r] >> 5)], 1u << (res[r] & 31));      // (fewer than k residues)
}
#endif
