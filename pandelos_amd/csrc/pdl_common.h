// pdl_common.h — shared declarations of the HIP implementation behind include/pandelos_amd.h.
// gfx950 only: wave = 64 lanes, 160 KiB LDS per CU, no other target is considered.
#pragma once

#include <atomic>
#include <chrono>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <cstdlib>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pandelos_amd.h"

#define PDL_WAVE 64

// A posting is {gene, count}; bit 31 of the count word says "opens a rank-group" (K-rle sets it, nothing takes it out): whoever
// reads a count masks it.
constexpr uint32_t PDL_COUNT_MASK = 0x7fffffffu;

// The workgroup barrier of every kernel here: all LDS operations of the wave have COMPLETED before it arrives.
// hipcc (ROCm 7.2, gfx950) leaves the `s_waitcnt lgkmcnt(0)` out in front of an `s_barrier` when the wave needs no LDS result
// any more — e.g. behind a run of no-return LDS atomics or stores — relying on the LDS pipe serving the CU's waves in order.
// On MI355X that does not hold across waves: with two or three 53-KB workgroups per CU the 2048-slot join tier read staged
// ranges and table slots of the row BEFORE (the wave in front of the barrier still had writes queued), a few wrong cells per
// pass on the last genomes of a 16-genome set, 0 with this wait in place.  The wait costs nothing
// when nothing is outstanding.
#ifdef __HIPCC__
__device__ __forceinline__ void pdl_sync() {
#ifndef PDL_PLAIN_SYNCTHREADS        // (defined only by the negative control of tests/test_isa.py: the barrier as hipcc emits it by itself)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}
// A lane's neighbour in the wave without a trip through the LDS crossbar: one DPP move (wave_shr:1 / wave_shl:1, gfx9).
// wave_prev_u32: lane l > 0 gets lane l - 1's v, lane 0 gets `first`; wave_next_u32: lane l < 63 gets lane l + 1's v, lane 63
// gets `last`.  Called with all 64 lanes active.
__device__ __forceinline__ uint32_t wave_prev_u32(uint32_t v, uint32_t first) {
    return (uint32_t) __builtin_amdgcn_update_dpp((int) first, (int) v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_next_u32(uint32_t v, uint32_t last) {
    return (uint32_t) __builtin_amdgcn_update_dpp((int) last, (int) v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ uint64_t wave_prev_u64(uint64_t v, uint64_t first) {
    return (uint64_t) wave_prev_u32((uint32_t) (v >> 32), (uint32_t) (first >> 32)) << 32 | wave_prev_u32((uint32_t) v, (uint32_t) first);
}
#endif

// ---- layout of the control block (pdl_ctx::scalars, u64 words): totals [16] | residue histogram [256] | per-genome cost ------
// Every use of a word is queued on the context's one stream, so two lives of a word cannot overlap as long as the later one
// starts behind the last kernel or read of the earlier one: each alias below says which stage that is.  A scan STORES its
// total (no clearing needed); the atomically added words are cleared by the stage that is about to add to them.
enum : size_t {
    PDL_CTL_RECORDS = 0,        // U: total of the dedup scan (K-rle); a multi-GPU finish uploads the gathered dictionary's count here
    PDL_CTL_FREE_1 = 1,         // no stage of a build uses it (cleared / uploaded with its neighbours); pdl_dist_preprocess_finish_ranges counts
                                //   the bad range tuples a peer sent here (k_tuple_check), before it uploads anything
    PDL_CTL_RANGES = 2,         // ranges built (total of the tile counts); sender-built lists: the tuples a rank received
    PDL_CTL_BAD_OFFSETS = 3,    // K-len: extra total of its apply functor (offsets that do not ascend)
    PDL_CTL_KSEQ_SUM = 4,       // k_genome_cost: sum of the genes' k-mer counts ...
    PDL_CTL_KMERS = 5,          // M: total of K-len's scan
    PDL_CTL_EMITTED = 6,        // K-order: emitted cells (total of the row-count scan)
    PDL_CTL_KSEQ_MAX = 7,       // ... their maximum ...
    PDL_CTL_KSEQ_NMIN = 8,      // ... and ~minimum (a max of complements, so that it starts at zero like the rest)
    PDL_CTL_MIRRORED = 9,       // K-order: mirrored cells (total of the mirror-count scan)
    PDL_CTL_COUNTERS = 10,      // GroupTileArgs::counters [4] of the range build:
    PDL_CTL_SHARED = 10,        //   [0] records in groups of two or more (U')
    PDL_CTL_GROUPS = 11,        //   [1] such groups
    PDL_CTL_OWN_COST = 12,      //   [2] lookups of this context's genes ("Total cost")
    PDL_CTL_REPEATS = 13,       //   [3] records whose k-mer repeats inside its gene
    PDL_CTL_SCAN_TOTAL = 15,    // total of every radix pass of pdl_sort_pairs: the sort runs in the middle of the range build, so
                                // no word the build keeps until its read at the end may live here
    PDL_CTL_LAST = 15,

    // second lives.  The range build's counters (10-13) are read by the host at the end of stage_ranges_and_costs /
    // pdl_run_dist_ranges; everything below that shares them runs before the build clears them or after that read.
    PDL_CTL_SLICE_COUNTERS = 12,// [4], 12-15: dist_slice_pipeline's COUNT pass (only its per-genome sums are wanted); behind the slice's
                                // sort, before the finish clears MIRRORED..LAST
    PDL_CTL_OUTBOX_TOTAL = 12,  // total of the outbox scan (pdl_run_dist_score_begin): scoring, the build has been read
    PDL_CTL_EDGES_1 = 13,       // K-bbh: totals of its two edge scans; runs on a scored context
    PDL_CTL_EDGES_2 = 14,
    PDL_CTL_LAZY_KSEQ_SUM = 13, // pdl_ensure_costs: where k_genome_cost's three statistics go when only its per-genome sums are
    PDL_CTL_LAZY_KSEQ_MAX = 14, //   wanted (max, ~min: 14, 15); after a build, with no sort in flight
    PDL_CTL_SELECT_TOTAL = 15,  // total of the multi-GPU selection scan, between K-rank and the slice's sort
    // K-fam (pdl_families.h) runs behind K-bbh's read of its totals, or on a caller's edges; k_fam_init clears FIRST..LAST, every
    // word is read before the call returns, and the sorts in the middle of it keep to SCAN_TOTAL
    PDL_CTL_FAM_FIRST = 10,
    PDL_CTL_FAM_BAD_IDS = 10,   // F-check: edges that name a gene id outside [0, N); read before F-cc starts ...
    PDL_CTL_FAM_RUNS = 10,      // ... then the total of the (label, genome) run scan (nobody reads it)
    PDL_CTL_FAM_NODES = 11,     // genes that are a node (stored by the family scan's apply functor); NODES..COLLIDING leave in one read
    PDL_CTL_FAM_FAMILIES = 12,  // F: total of the family scan
    PDL_CTL_FAM_COLLIDING = 13, // families that hold a collision
    PDL_CTL_FAM_INTRA = 14,     // a caller's edges: intra-genome edges before de-duplication (total of their compaction, the sort's count)
    PDL_CTL_FAM_LAST = 14,

    PDL_CTL_HIST = 16,          // residue histogram [256]
    PDL_CTL_GCOST = 16 + 256,   // per-genome cost [G] (+ [G] lookups above the diagonal, multi-GPU)
};
// ---- layout of pdl_ctx::rm.ctl (u64 words): what a removal (pdl_remove.h) leaves for the host's one read before the context
// changes.  A block of its own: a refused removal must not have touched a word of `scalars`.  Cleared by pdl_run_remove.
enum : size_t {
    PDL_RM_GENES = 0,           // genes that stay: total of the R-map scan
    PDL_RM_KMERS = 1,           // their k-mer occurrences: total of the compaction's tile scan
    PDL_RM_GONE_RESIDUES = 2,   // residues of the genes that leave (added up by R-map)
    PDL_RM_SEEN = 4,            // u32 [256] (128 words): digit d occurs in a key that stays (R-alpha; every workgroup stores the same 1)
    PDL_RM_WORDS = 4 + 128,
};

// ---- layout of pdl_ctx::pb.ctl (u64 words): K-place (pdl_place.h).  A block of its own: a placement only reads the context, so
// no word of `scalars` but the sort's SCAN_TOTAL may move.  Cleared at the start of every run of the placement stages (a single
// query's, or a chunk's of a batch: the counts are then the chunk's); each word has one life.
// One reader each on the host (the PinReads of pdl_place.h).  On the device a count is read only where it bounds a later stage's
// grid instead of a host read in between: INTRA and BASE_EDGES by their sorts, BASE_EDGES / BASE_PAIRS as the d_n of the scans behind
// them, BASE_PAIRS and GROUPS by k_place_base_off, NODES by k_place_clique.
enum : size_t {
    PDL_PL_BAD_EDGES = 0,       // P-check (a caller's list, pdl_run_place_edges): edges with an id outside [0, N + n) or with both ends below N; read before the run
    PDL_PL_EDGES_1 = 1,         // K-bbh over the query block: phase-1 cells (two edges each) and phase-2 cells, totals of the two
    PDL_PL_EDGES_2 = 2,         //   edge scans; read together before P-cc
    PDL_PL_INTRA = 3,           // a caller's list: query-query edges before de-duplication (total of their compaction, the sort's count)
    PDL_PL_NODES = 4,           // query genes that are a node (stored by the group scan's apply functor); NODES..MEMBERS leave in one read
    PDL_PL_GROUPS = 5,          // groups: total of the group scan
    PDL_PL_BASE_EDGES = 6,      // edges with a base end (total of their compaction, the sort's count)
    PDL_PL_BASE_PAIRS = 7,      // distinct (group, base component) pairs: total of the run-head scan
    PDL_PL_MEMBERS = 8,         // genes of the base components that groups of two or more of them fuse (total of the member scan)
    PDL_PL_WORDS = 16,
};

// ---- layout of pdl_ctx::pb.bctl (u64 words): K-place for a batch (pdl_place_batch.h).  The words of a chunk of queries in front
// of the placement stages; those stages count in the PDL_PL_* words above, once per chunk (NODES .. MEMBERS are the chunk's, the
// queries' shares are cut out of the arrays on the host).  Cleared at the start of every chunk; each word has one life and one
// reader on the host.
enum : size_t {
    PDL_PB_EDGES_1 = 0,         // K-bbh over the chunk's cells: phase-1 cells (two edges each) and phase-2 cells of all its queries,
    PDL_PB_EDGES_2 = 1,         //   totals of the two edge scans; read together with the prefixes at every query's first cell
    PDL_PB_BAD_QUERY = 2,       // PB-check (callers' lists): number of failing queries behind the first one that fails, as
                                //   n_queries - (its index), 0 when none fails (an atomicMax finds the FIRST); read before any id is used
    PDL_PB_WORDS = 4,
};

static_assert(PDL_CTL_EDGES_2 == PDL_CTL_EDGES_1 + 1 && PDL_PL_EDGES_2 == PDL_PL_EDGES_1 + 1 && PDL_PB_EDGES_2 == PDL_PB_EDGES_1 + 1,
              "K-bbh's two totals are neighbours: one pointer names them (bbh_edges, bbh_read_counts)");

// ---- layout of pdl_ctx::join_ctr (u32 words): cursors and counters of one scoring pass, cleared by score_join ---------------
// A tier draws rows through its cursor and lists the rows it hands on; the count of that list is the next tier's work size.
enum : uint32_t {
    PDL_JC_CURSOR_T1 = 0,       // cursor of tier 1
    PDL_JC_ROWS_T2 = 1,         // rows tier 1 handed to tier 2
    PDL_JC_CURSOR_T2 = 2,
    PDL_JC_ROWS_T3 = 3,         // rows tier 2 handed to tier 3 (a dataset of very long genes: all rows, uploaded)
    PDL_JC_CELLS = 4,           // u64 (words 4-5): staging cells reserved
    PDL_JC_ERRORS = 6,          // internal consistency violations (join, inbox filing)
    PDL_JC_CURSOR_T3 = 7,
    PDL_JC_WIDE_ROWS = 9,       // rows of more than 256 cells seen by K-order
    PDL_JC_RELOADS = 10,        // entries of the put-aside lists that had to be loaded again
    PDL_JC_CURSOR_T0 = 11,      // cursor of tier 0 (the partition tier)
    PDL_JC_ROWS_T0B = 12,       // rows it handed to its second form
    PDL_JC_CURSOR_T0B = 13,
    PDL_JC_ROWS_T1 = 14,        // rows the second form handed to tier 1
    PDL_JC_WORDS = 16,          // (whole 16-byte words: cleared as uint4)
};
// What k_gather_u32 appends to the gathered cell offsets (fin_off -> task_off) for the one read after K-order.  Words 0-7 and
// RELOADS sit where join_ctr has them, so one reader (JoinCounters) serves this tail and a direct read of join_ctr.
enum : uint32_t {
    PDL_JT_CTR_WORDS = 8,       // join_ctr[0..8) as they are
    PDL_JT_EMITTED = 8,         // u64 (words 8-9): scalars[PDL_CTL_EMITTED]
    PDL_JT_RELOADS = PDL_JC_RELOADS,
    PDL_JT_ROWS_T1 = 11,        // join_ctr[PDL_JC_ROWS_T1]
    PDL_JT_WORDS = 12,
};
static_assert(PDL_JC_ROWS_T1 < PDL_JC_WORDS && PDL_JC_RELOADS < PDL_JT_WORDS && PDL_JC_CURSOR_T3 + 1 == PDL_JT_CTR_WORDS, "join counter layout");

// ---- error plumbing -------------------------------------------------------------------------
struct pdl_error {
    int code;
    std::string msg;
};

#define PDL_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            throw pdl_error{PDL_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)}; \
        }                                                                                       \
    } while (0)

#define PDL_FAIL(code_, ...)                                  \
    do {                                                      \
        char _b[512];                                         \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                \
        throw pdl_error{(code_), std::string(_b)};            \
    } while (0)

// ---- device buffer ----------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    void alloc(size_t n) {            // grows only; contents undefined
        if (n <= bytes && p) return;
        release();
        size_t want = n ? n : 16;
        PDL_HIP(hipMalloc(&p, want));
        bytes = want;
    }
    void release() {
        if (p) (void) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~DevBuf() { release(); }
    void grow_keep(size_t n, hipStream_t st) {   // grows and keeps the contents (a device copy on `st`, waited for)
        if (n <= bytes && p) return;
        void *q = nullptr;
        PDL_HIP(hipMalloc(&q, n));
        if (p && bytes) {
            PDL_HIP(hipMemcpyAsync(q, p, bytes, hipMemcpyDeviceToDevice, st));
            PDL_HIP(hipStreamSynchronize(st));
            (void) hipFree(p);
        }
        p = q;
        bytes = n;
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// ---- pinned host buffer: grows only, with a quarter of headroom (a need that creeps up does not allocate every time); contents
// undefined.  A DMA target: no staging by the runtime and no page of a fresh vector to touch.
struct PinBuf {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    void alloc(size_t n) {
        if (n <= bytes) return;
        release();
        PDL_HIP(hipHostMalloc((void **) &p, n + n / 4, hipHostMallocDefault));
        bytes = n + n / 4;
    }
    void release() {
        if (p) (void) hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    ~PinBuf() { release(); }
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
};

// workgroups of 256 threads over n items
inline dim3 grid256(uint64_t n) { return dim3((uint32_t) ((n + 255) / 256)); }

// v = the `count` values at d, once the stream gets there: sizes the vector and queues the copy
template <class T> inline void copy_down(hipStream_t st, std::vector<T> &v, const void *d, size_t count) {
    v.resize(count);
    if (count) PDL_HIP(hipMemcpyAsync(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, st));
}

// K-bbh's buffers (pdl_bbh.hip), one set per owner — the context's for its genome tasks, K-place's for a query block or a chunk:
// kind u8 [Z] | tab: inter_max, thr, the two prefix lists [Z + 1] and the blocks' first cells with their picked prefixes |
// e_*: the edges, phase 1 from 0 (room for 2 Z), phase 2 from 2 Z (room for Z).  The context's e_src / e_dst are read by K-fam long
// after a placement has run over its own set.
struct BbhBufs { DevBuf kind, tab, e_src, e_dst, e_score; };

// K-bbh's counts as one read brings them — t1 / t2: the cells of the two kinds; picks [2][nb + 1] (nullptr: one block): the cells
// of each kind before every block's first cell at[i], of Z — to every block's first phase-1 edge (two per cell) and first phase-2
// edge, e1 / e2 [nb + 1]; a block that starts at Z takes the totals.  PDL_ERR_DEVICE for counts that cannot be: totals above Z,
// offsets that decrease or pass the totals (block0: the caller's index of block 0, for the message).
inline void bbh_cut_blocks(const char *who, uint64_t t1, uint64_t t2, const uint32_t *picks, const uint32_t *at, uint32_t nb, uint64_t Z, uint32_t block0,
                           std::vector<uint64_t> &e1, std::vector<uint64_t> &e2) {
    if (t1 > Z || t2 > Z) PDL_FAIL(PDL_ERR_DEVICE, "%s: %llu + %llu edge cells of %llu cells", who, (unsigned long long) t1, (unsigned long long) t2, (unsigned long long) Z);
    e1.assign((size_t) nb + 1, 0); e2.assign((size_t) nb + 1, 0);
    for (uint32_t i = 0; i <= nb; i++) {
        const bool past = !picks ? i == nb : at[i] >= Z;
        e1[i] = 2 * (past ? t1 : picks ? (uint64_t) picks[i] : 0); e2[i] = past ? t2 : picks ? (uint64_t) picks[nb + 1 + i] : 0;
    }
    for (uint32_t i = 0; i < nb; i++)
        if (e1[i + 1] < e1[i] || e2[i + 1] < e2[i] || e1[i + 1] > 2 * t1 || e2[i + 1] > t2) PDL_FAIL(PDL_ERR_DEVICE, "%s: inconsistent edge offsets at block %u", who, block0 + i);
}

// a typed window into someone else's device allocation
struct DevView {
    void *p = nullptr;
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// ---- alphabet / rank parameters (library.cpp:56-64, 88-132) -----------------------------------
struct RankParams {
    uint8_t rank_values[256];
    uint64_t last_multiplier;
    uint32_t base;          // B (kept as the reference's unsigned char value)
    uint32_t k;
    uint32_t rank_bits;     // bits of a rank as rank_init sees them: what the sort by rank goes over (the reference's rank_byte_order bytes)
    uint32_t hash_fallback;
    uint32_t key_bits;      // bits a rank can really occupy: rank_bits — or 64 where B^k wrapped past 2^64 UNNOTICED by rank_init's overflow test
                            // (library.cpp:104-111 looks one multiplication ahead with wrapped products: 22 letters, k = 15), the ranks being the polynomial mod 2^64
};
#define RABIN_MODULO 18446744073709551557ULL   /* 2^64 - 59, library.cpp:19 */
// what a kernel needs to take a key of an exact alphabet apart into its digits (pdl_rekey.h: rk_plan makes it, rk_items / rk_one read it)
struct RkArgs {
    uint32_t k, base;           // of the keys that come in
    uint32_t nparts, h;         // parts a key is cut into (1 for 32-bit keys), digits of every part but the last
    uint64_t magic;             // RmDigits::magic of `base`
    uint64_t part_div;          // B^h
    uint64_t part_magic;        // floor(2^64 / B^h)
    uint32_t entries;           // k * base
};
// base^k < 2^64, in exact arithmetic (the reference's own test compares wrapped products and lets some wraps through: 20 letters
// at k = 15 wrap unnoticed to a 64-bit rank_bits).  The one place that says so: rank_init_host's key_bits and rk_exact ask here.
inline bool pow_fits_u64(uint32_t base, uint32_t k) {
    unsigned __int128 p = 1;
    for (uint32_t i = 0; i < k; i++) { p *= base; if (p >> 64) return false; }
    return true;
}

// The width of the context's keys as a type: f(uint64_t{}) or f(uint32_t{}), for a generic lambda that names it decltype(tag).
template <class F> inline decltype(auto) pdl_with_key(bool key64, F &&f) {
    if (key64) return f(uint64_t{});
    return f(uint32_t{});
}
// ... and of a base's keys beside those of a superset alphabet's (option "query_rekey"): f(KeyB{}, KeyQ{}).  B'^k >= B^k, so
// 64-bit base keys never meet 32-bit union keys: that pair is not instantiated, and seeing it is an error of the plan.
template <class F> inline void pdl_with_keys_up(bool base64, bool union64, F &&f) {
    if (base64 && !union64) PDL_FAIL(PDL_ERR_DEVICE, "query_rekey: the base's keys are 64 bits wide and the union's 32 — a superset alphabet cannot need fewer");
    if (!union64) f(uint32_t{}, uint32_t{});
    else pdl_with_key(base64, [&](auto key_b) { f(key_b, uint64_t{}); });
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    bool used = false;
};

// device time of a call = its stretches of device work between the host's reads, each between a pair of events (N at most).
// The timer owns its events: made at the first start(), destroyed with the struct that holds it.
template <int N> struct EventSpans {
    hipEvent_t ev[2 * N] = {};
    hipStream_t st = nullptr;
    int n = 0;
    void start(hipStream_t s) { st = s; n = 0; for (hipEvent_t &e : ev) if (!e) PDL_HIP(hipEventCreate(&e)); }
    void begin() { PDL_HIP(hipEventRecord(ev[2 * n], st)); }
    void end() { PDL_HIP(hipEventRecord(ev[2 * n + 1], st)); n++; }
    float ms(int i) const { float v = 0.f; return i < n && hipEventElapsedTime(&v, ev[2 * i], ev[2 * i + 1]) == hipSuccess ? v : 0.f; }     // (after the stream has been synchronized)
    float total_ms() const { float total = 0.f; for (int i = 0; i < n; i++) total += ms(i); return total; }
    EventSpans() = default;
    EventSpans(const EventSpans &) = delete;
    EventSpans &operator=(const EventSpans &) = delete;
    ~EventSpans() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};
using QSpans = EventSpans<4>;      // (a query that is asked for its letters has one host read more)
// Everything a struct of work buffers holds goes back and its bookkeeping starts again: the members release themselves, so a
// member added to the struct is released without being named anywhere else.
template <class T> inline void pdl_renew(T &x) { x.~T(); new (&x) T(); }

// what one run of K-fam (pdl_families.h) leaves on the host: pdl_families without the C allocation
struct pdl_fam_result {
    uint32_t sequences = 0, nodes = 0, families = 0, colliding = 0;
    std::vector<uint32_t> component_of, family_off, family_genes;
    std::vector<uint8_t> is_node, collides;
    float device_ms = 0.f;
};

// what one run of K-place (pdl_place.h) leaves on the host: pdl_placement without the C allocation
struct pdl_place_result {
    uint32_t sequences = 0, n_query = 0, genomes = 0, edges_phase1 = 0, groups = 0;
    uint32_t novel = 0, joined = 0, bridging = 0, colliding = 0, unplaced = 0;
    std::vector<uint32_t> family_of, group_label, group_query_off, group_query, group_base_off, group_base;
    std::vector<uint8_t> is_node, group_collides;
    float device_ms = 0.f;
    // A query's edges are the C arrays the caller gets (malloc, `n` entries each, phase 1 then phase 2; pdl_api.hip's fill_placement
    // takes them): a single query's come down into them, a batch's are cut out of the chunk's pinned staging in one pass.  A
    // caller's list leaves them empty.
    struct CEdges {
        int32_t *src = nullptr, *dst = nullptr; float *score = nullptr; uint64_t n = 0;
        CEdges() = default;
        CEdges(const CEdges &) = delete;
        CEdges &operator=(const CEdges &) = delete;
        CEdges(CEdges &&o) noexcept { *this = std::move(o); }
        CEdges &operator=(CEdges &&o) noexcept {
            if (this != &o) { drop(); src = o.src; dst = o.dst; score = o.score; n = o.n; o.release(); }
            return *this;
        }
        void release() { src = dst = nullptr; score = nullptr; n = 0; }      // (the arrays have a new owner)
        void drop() { free(src); free(dst); free(score); release(); }
        ~CEdges() { drop(); }
    } c_edges;
};
// the base network's families as K-place reads them (device pointers): the context's own, uploaded once from c->fam, or a caller's
struct PlaceBase {
    const uint32_t *comp = nullptr, *fam_off = nullptr, *fam_genes = nullptr, *fam_of_label = nullptr, *genome_of = nullptr;
    const uint8_t *is_node = nullptr, *collides = nullptr;
    uint32_t N = 0, G = 0;      // G: the query's genome id (every base genome id is below it)
};
// ... where they lie on the device, with the family of every label as the host derived it (kept alive for the asynchronous copy)
struct BaseBufs {
    DevBuf comp, is_node, collides, fam_off, fam_genes, fam_of_label;
    std::vector<uint32_t> of_label;
    PlaceBase view(uint32_t N, const uint32_t *genome_of, uint32_t G) const {
        PlaceBase B;
        B.comp = comp.as<uint32_t>(); B.is_node = is_node.as<uint8_t>(); B.collides = collides.as<uint8_t>();
        B.fam_off = fam_off.as<uint32_t>(); B.fam_genes = fam_genes.as<uint32_t>(); B.fam_of_label = fam_of_label.as<uint32_t>();
        B.genome_of = genome_of; B.N = N; B.G = G;
        return B;
    }
};
// ... and as the host holds them: a pdl_fam_result's vectors or a caller's pdl_families
struct FamView {
    uint32_t N, families, nodes;
    const uint32_t *component_of, *family_off, *family_genes;
    const uint8_t *is_node, *collides;
};
// of_label[label] = the family whose smallest member (its first) the label is; 0 for every other gene
inline void fam_of_label(const FamView &f, std::vector<uint32_t> &of_label) {
    of_label.assign(f.N, 0);
    for (uint32_t i = 0; i < f.families; i++) of_label[f.family_genes[f.family_off[i]]] = i;
}
// what the host knows of one query of a batch before the device is asked (pdl_query_batch.h)
struct QBQuery {
    uint32_t g0, n;                 // its genes in the caller's arrays
    uint64_t Rq, Mq;                // residues, k-mers
    uint64_t bytes;                 // device memory the stages before the join need for it (the chunking's weight)
};
// What the device half of a single query (pdl_query.h, pdl_run_query_device) or of a chunk of a query batch (pdl_query_batch.h,
// pdl_run_query_chunk_device) leaves in HBM, until the context's next query: Z ordered cells, query after query, in five arrays of
// `cap` (scores, percs, tr_percs, row, column) at `cells`; MS [genes][G + 1] by the run's gene; the queries' CM slices [N + n_q], query
// q's at q * N + gene_begin[q].  A single query is the run of one query, gene_begin = {0, n}, which nothing on the device asks for.
struct pdl_query_cells {
    const float *cells = nullptr, *MS = nullptr, *CM = nullptr;
    uint64_t Z = 0, cap = 1;
    uint32_t nq = 0, genes = 0;
    std::vector<uint32_t> gene_begin;                            // [nq + 1] first gene of every query ...
    const uint32_t *d_gene_begin = nullptr;                      // ... and on the device (a chunk's)
    std::vector<uint64_t> cells_of, records, matched, cost;      // [nq]
    uint64_t residues = 0, kmers = 0;                            // of the whole run
    const QSpans *spans = nullptr;                       // the run's stretches of device work ...
    float device_ms() const { return spans->total_ms(); }        // ... their time, once the stream has been waited for
    // query q as the caller's pdl_query_info reports it, with the sizes the host knew of it and its share of the device time
    void info_of(uint32_t q, uint64_t q_residues, uint64_t q_kmers, float ms, pdl_query_info *fi) const {
        *fi = pdl_query_info{};
        fi->residues = q_residues; fi->kmer_occurrences = q_kmers; fi->records = records[q]; fi->matched_records = matched[q];
        fi->genome_cost = cost[q]; fi->device_ms = ms;
    }
};

// The stages of a multi-GPU build and pass, in the order the pdl_dist_* calls walk them (DESIGN.md section 16 has who sets and
// who requires each); `none`: no multi-GPU build has gone as far as its slice.
enum class DistStage : int { none, slice_built, adopted, joined, scored };

// ---- the context --------------------------------------------------------------------------------
struct pdl_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t flags = 0;
    std::string err;
    std::mutex mu;

    // inputs (device)
    const uint8_t *d_res = nullptr;
    const uint64_t *d_off = nullptr;
    const uint32_t *d_gen = nullptr;
    DevBuf in_res, in_off, in_gen;
    DevBuf own_gen;       // u32 [N] genome ids after an append: the context's own copy (the caller's input may be gone by then)

    // device-resident input: genome ids (and the two ends of the offsets) come to the host through this pinned buffer while the
    // first kernels already run; the genome layout is built behind them (pdl_finish_layout)
    uint32_t *gen_pin = nullptr; size_t gen_pin_words = 0;
    hipEvent_t ev_gen = nullptr;
    bool layout_deferred = false;

    bool preprocessed = false;
    bool only_complexity = false;
    uint32_t N = 0, G = 0;
    uint64_t R = 0, M = 0, U = 0, Ushared = 0, NG = 0, P = 0, sum_kseq = 0, max_kseq = 0, min_kseq = 0;
    uint64_t Urepeat = 0;          // dictionary records with a count >= 2 (the k-mer repeats inside the gene): the "heavy" lookups of the join come from these
    RankParams rp{};

    // K-ingest (pdl_ingest.hip): the input a .faa file was parsed into, and the two pinned staging buffers it travelled through
    DevBuf ing_res, ing_off, ing_gen;
    uint8_t *ing_pin[2] = {nullptr, nullptr};    // [0]: the pinned staging buffer of the ingest (the whole file's residues)
    size_t ing_pin_bytes = 0;
    hipEvent_t ing_ev[2] = {nullptr, nullptr};
    hipStream_t ing_stream = nullptr;
    std::vector<uint64_t> ing_h_off;
    std::vector<uint32_t> ing_h_gen;
    std::vector<std::string> ing_genome_names;
    uint64_t ing_R = 0;
    bool ingested = false;

    // per sequence
    DevBuf kseq_len;      // u32 [N]
    DevBuf gene_len;      // u32 [N] residues of each gene (K-len stores it beside kseq_len, which forgets genes shorter than k): a removal's pdl_cost.residues
    DevBuf kmer_off;      // u64 [N+1]
    DevBuf cost;          // u64 [N]   total_visited
    std::vector<uint64_t> h_genome_cost;

    // sort buffers / dictionary
    DevBuf keys_a, keys_b, vals_a, vals_b, sort_tmp;
    bool key64 = false;
    DevBuf recpos;        // u32 [U+1] position of each record's first occurrence in the sorted stream
    DevBuf post;          // uint2 [U] {seq, count}  — the dictionary postings, rank-group major (bit 31 of count: opens a rank-group; it stays, readers mask it)
    DevBuf ranges;        // uint4 [U'] {group start, group length, own count, 0}, gene major
    const uint2 *ranges8 = nullptr;   // packed 8-byte ranges (inside `scratch`, the gene sort's output) when the dataset allows: see GroupTileArgs::pay8
    DevBuf head_bits;     // u64 [U / 64] "opens a rank-group" per record, kept by K-ranges for the per-gene costs made on demand
    bool costs_ready = true;          // cost[] / h_genome_cost hold the per-gene / per-genome lookups (packed ranges: made on first request)
    DevBuf seq_off;       // u32 [N+1] range list of each gene
    bool upper_only = false;  // ranges hold only the columns above the row: the join mirrors every cell
    DevBuf scan_tmp;      // block sums of the scans
    DevBuf lb_tile, lb_chunk, lb_ctr;     // decoupled look-back (pdl_scan.h): status words of tiles / chunks, ticket + arrival counters
    uint32_t lb_epoch = 0;
    bool opt_low_memory = false;          // batches of genomes on a large set: build buffers released after the dictionary, small HBM tables for tier 3
    bool reshard_pending = false;         // pdl_set_genome_shard named genomes the range lists on the device do not cover: they are built before the next scoring pass
    bool opt_onepass_scan = false;        // scans in one launch (decoupled look-back) instead of three: measured 3-10 % slower per scan on MI355X, kept as an option
    int opt_order_offsets = 2;            // K-order's two offset scans: 2 = one launch of several workgroups (k_order_offsets), 1 = of one workgroup, 0 = the four launches of two scans
    uint32_t opt_order_offsets_rows = 1u << 17;   // ... for at most so many task rows (at most OO_MAX_ROWS; tests lower it)
    int opt_order_subwave = 1;            // K-order: several short rows per wave, each in a segment of lanes: 1 = the default width, 16 | 32 = that many lanes, 0 = a wave per row
    bool opt_order_wide_merged = true;    // ... with the wide rows' workgroups behind them in the same launch; 0: k_order_rows in a launch of its own
    int opt_fused_glue = 1;               // small launches that share one: row descriptors + clearing (scoring), K-cost + K-seq-offsets (build); n > 1: also K-len with the control block's clearing, for up to min(n, KL_MAX_GENES) genes (measured: does not pay); 0: each its own
    bool opt_lean_radix = true;          // radix passes: offsets in one launch (k_rs_offsets), the rank sort's first histogram filed by K-rank; 0: a histogram and a three-launch scan per pass
    bool opt_lean_records = true;        // the build's record passes load each k-mer once: K-rle in kernels of its own (k_rle_tile_sums / k_rle_apply), the middle launch of a three-launch scan with its sums staged through LDS (k_scan_tile_scan_lds); 0: the former kernels
    DevBuf scratch;       // transient buffers of the range build
    DevBuf scalars;       // control block, u64: totals [16] | residue histogram [256] | per-genome cost [G] (PDL_CTL_*, above)

    // genome / task layout (host and device)
    std::vector<uint32_t> h_genome_of;
    std::vector<uint32_t> h_genome_row_off;   // [G+1] into h_genome_rows
    std::vector<uint32_t> h_genome_rows;      // gene ids grouped by genome, ascending inside a genome
    std::vector<uint32_t> shard;              // genomes scored by this context (ascending)
    bool shard_set = false;
    std::vector<uint32_t> dict_shard;         // genomes whose genes have range lists on the device (empty = all)
    DevBuf seq_in_shard;                      // u8 [N] gene belongs to dict_shard
    DevBuf own_iv;                            // uint2 [intervals] the same as sorted gene-id intervals, when genomes are consecutive id ranges
    std::vector<uint2> h_own_iv;
    std::vector<uint8_t> h_seq_in_shard;      // its host copy (kept alive for the asynchronous upload)

    // scoring results (device)
    bool scored = false;
    uint32_t n_task_rows = 0;
    std::vector<int32_t> h_local_genome;      // [G] genome -> index in shard or -1
    std::vector<uint32_t> h_task_row_off;     // [shard+1] task position of each shard genome's first row
    std::vector<uint64_t> h_cell_off;         // [shard+1] first cell of each shard genome
    // task layout on the device: one allocation, one upload from a pinned staging buffer (pdl_prepare_tasks)
    DevBuf task_blob;
    uint32_t *task_pin = nullptr; size_t task_pin_words = 0;
    hipStream_t copy_stream = nullptr; hipEvent_t ev_tasks = nullptr, ev_entry = nullptr;     // uploads of the task layout, beside the build's stream
    DevView task_rows;    // u32 [n_task_rows] gene id of each task position
    DevView task_lg;      // u32 [n_task_rows] shard-local genome index
    DevBuf row_desc;      // uint4 [n_task_rows] {task position, gene, first range, ranges} in processing order
    DevBuf MS;            // f32 [n_task_rows][G]      max_genome_score rows
    DevBuf CM;            // f32 [shard][N]            max_genome_score_col per genome task
    DevBuf row_base, row_cnt, fin_off;   // u32 [n_task_rows(+1)]
    DevBuf st_score, st_perc, st_tr, st_col, st_first;   // staging cells (unordered inside a row)
    uint64_t st_cap = 0;
    DevBuf c_score, c_perc, c_tr, c_row, c_col;          // final cells, task order + emission order
    uint64_t Z = 0;
    DevBuf join_ctr;      // u32 [PDL_JC_WORDS] cursors / counters of the join (PDL_JC_*)
    DevBuf overflow_rows; // u32 [n_task_rows]
    DevBuf gene_info;             // uint4 [N] {k-mers, genome, task position, shard-local genome}: one load per candidate column in finalize
    DevBuf join_defer;            // filter tiers of the join: per workgroup, the first sightings put aside
    DevBuf glb_table;     // HBM tables of the overflow pass
    bool glb_clean = false;   // all-zero where the layout below has its tables (k_join_hbm leaves them that way; its lists it leaves as they were)
    uint32_t glb_cols = 0, glb_slots = 0;    // the layout the tables were last cleared or run for: columns (N), workgroups,
    bool glb_wide = false;                   // 32-bit counters — under another one the old lists lie where the new tables do
    DevBuf row_desc2;     // descriptors of the rows handed from tier 1 to tier 2
    DevBuf mirror_cnt, mirror_ref;   // mirror mode (see pdl_join.hip); mirror_ref: the mirrored cells (MCell), per row
    DevView taskpos_of;                      // u32 [N] task position of every gene (0xffffffff: not a row of this context)
    std::vector<uint32_t> h_fin;
    bool tasks_ready = false;  // task layout uploaded for the current shard
    DevBuf scratch2;      // small transient device scratch (interval histogram, per-genome lookups)
    DevBuf task_off;      // u32 [shard+1] task offsets | gathered cell offsets + the counters behind them (PDL_JT_*)
    int cus = 0;
    uint32_t join_occ[16] = {};   // workgroups per CU of the join's kernels, by entry of pdl_join.hip's tier table (0: not asked yet)

    // K-bbh (pdl_bbh.hip): network edges of every genome task, on the host after the first pdl_compute_edges
    bool edges_valid = false;
    BbhBufs bbh;
    PinBuf edge_mirror;                       // src1 | dst1 | score1 (phase 1) | src2 | dst2 | score2 (phase 2)
    uint64_t n_edges = 0, n_edges1 = 0;
    std::vector<uint64_t> h_edge1, h_edge_off;   // [shard+1] first phase-1 / phase-2 edge of every genome task

    // tuning / test switches (pdl_set_option)
    int opt_tier1 = -1;           // -1: by genome count
    int opt_tier0 = -1;           // the partition tier in front of tier 1: -1 by row length, 0 off, 1 on
    int opt_sift_threshold = 1;   // tier 0's sift: 1 = counters against the set's validity threshold (bitmaps where that is below PT_SIFT_T_MIN), 0 = counters at threshold 2 (tests)
    bool opt_tiny_tier2 = false;
    bool opt_stage_timers = true; // per-stage HIP events (pdl_timings' stage fields); the totals and the join's are always taken
    int opt_grid_pct = 0;         // > 0: tier-1 grid as a percentage of what fits the chip (experiments)
    bool opt_host_mirror = true;
    uint64_t opt_staging_cap = 0; // 0: estimate
    bool opt_aside_test_reload = false;   // test switch: the next pass with 8-byte put-aside entries counts as one that saw a reload

    // multi-GPU (pdl_dist_*): this context is rank `rank` of `world`; the postings live in caller-owned memory
    bool dist = false;
    uint32_t world = 1, rank = 0;
    DistStage dist_stage = DistStage::none;   // none | slice built | dictionary adopted | join done, outbox listed | scored
    uint2 *post_ext = nullptr;    // the all-gathered dictionary (caller's buffer), used instead of `post`
    uint64_t U_slice = 0, M_slice = 0;
    std::vector<uint32_t> h_owner;            // [G] rank of every genome
    std::vector<uint64_t> h_upper_cost;       // [G] lookups above the diagonal per genome (what a rank's join walks)
    std::vector<uint64_t> h_run_weights;      // [G] the same inside this rank's run of the dictionary (summed over ranks: the deal's weights)
    std::vector<uint64_t> h_run_costs;        // [G] lookups as the reference counts them, inside this run (summed over ranks: "Genome g cost")
    // sender-built range lists (pdl_dist_preprocess_ranges / _finish_ranges): every rank makes the range tuples of ITS run and
    // files them by the rank that owns the gene; the owners only sort what they receive
    bool dist_sender = false;                 // the range lists of this build came from the senders (per-gene costs are not kept then)
    int dist_tail = -1;                       // last rank with a non-empty interval (known to every rank: the cuts depend on the input only)
    uint64_t run_base = 0, dist_total = 0;    // first record of this run in the gathered dictionary; records of all runs
    DevBuf seq_owner;                         // u8 [N] rank that owns the gene
    DevBuf tuple_off;                         // u32 [world + 1] where each destination's tuples start in the outbox
    std::vector<uint64_t> h_tuple_counts;     // [world]
    uint32_t *dist_out_keys = nullptr;        // the outbox (inside `scratch`): (owner << 24 | gene), packed range
    unsigned long long *dist_out_ranges = nullptr;
    uint64_t dist_out_total = 0, dist_run_counters[3] = {0, 0, 0};     // shared records, groups, repeat statistic of this run
    DevBuf owner_of_genome;                   // u32 [G]
    DevView local_genome;                     // u32 [G] index in the shard, 0xffffffff for other ranks' genomes
    DevBuf outbox;                            // pdl_dist_cell [remote mirrored cells], grouped by destination rank
    DevBuf outbox_tab;                        // u32 [workgroups][world] counts, then offsets
    std::vector<uint64_t> h_outbox_counts;    // [world]
    uint64_t st_local = 0;                    // staging slots below this hold the cells of this rank's own rows
    uint64_t n_inbox = 0;
    uint32_t order_grid1 = 0;

    // K-query: what the stages a single query and a chunk of a batch share (pdl_query.h: q_dictionary .. q_join_and_order) work on —
    // the run's genes, its dictionary, the match's output, the rows, the control words, the maxima, the join's staging, the cells
    struct QStageBufs {
        DevBuf res, off, koff, kseq, keys_a, keys_b, vals_a, vals_b, recpos, post, desc, gkey, rec_sorted, row_lookups, row_off,
               ctl, MS, CM, row_base, row_cnt, fin_off, rowid, overflow, st, cells;
        QSpans spans;                                // up to three stretches of device work (four with option "query_rekey")
    };
    // pdl_query_scores (pdl_query.h): the query's own buffers, reused across queries, released at the next preprocess or destroy
    struct QueryBufs : QStageBufs {
        DevBuf fold, hbm;
        bool hbm_clean = false;                      // hbm holds hbm_slots tables laid out for hbm_cols columns, in their clean state
        uint32_t hbm_cols = 0, hbm_slots = 0;
        // option "query_rekey" (a single query's and a chunk's alike): the union's rank table and the two plans between the base's
        // alphabet and the union's, as the host decided them (pdl_query_rekey_plan, pdl_dict.hip), and Q-rebase's output
        struct Rekey {
            RankParams rp{};                         // the union's
            bool key64 = false;
            RkArgs up{}, down{};                     // base -> union (the fold's two ranks), union -> base (Q-rebase)
            std::vector<uint64_t> h_up, h_down;      // their tables (kept alive for the asynchronous uploads)
            std::vector<uint32_t> h_down32;
            uint32_t absent[8] = {};                 // digits of the union's alphabet that are letters the base lacks
            DevBuf up_table, down_table;
            DevBuf up3;                              // u64 [3]: the base's bmax and its last two records' ranks, in the union's alphabet
            DevBuf bkey, none;                       // per query record: its key in the base's alphabet | 1: it holds a letter the base lacks
            EventSpans<1> span;                      // Q-rebase alone (option "stage_timers")
        } rk;
    } qb;
    // pdl_query_batch (pdl_query_batch.h): the buffers of one chunk of queries, reused across chunks and calls, released with qb's
    // (the HBM tables of the join's last tier and their bookkeeping are qb's: a batch and a single query find each other's clean)
    struct QueryBatchBufs : QStageBufs {
        DevBuf gene_begin, res_begin, gene_query, qkey, perm, srank, spost, seg_off, folds;      // the layout; the segments
        PinBuf stage;                               // host staging of a chunk's cells and maxima, or of its edges (the blocks are cut out of it)
    } qbb;
    uint64_t opt_query_batch_bytes = 1ull << 30;    // pdl_query_batch: device bytes one chunk of queries may take before its join
    bool opt_query_rekey = false;                   // queries and placements accept letters the base lacks (pdl_query.h, Q-rebase)
    pdl_query_rekey_info qrk_call{}, last_query_rekey{};    // what the call under way / the last successful one of the four did about letters
    pdl_query_join_info qj_call{}, last_query_join{};       // ... and which way its rows took through the join (pdl_query.h, Q-join)
    // K-fam (pdl_families.h): work buffers of a run (grown as needed, shared by pdl_compute_families and pdl_families_of_edges) and
    // the context's own families, kept on the host until the edges change (pdl_run_bbh_all drops them)
    struct FamBufs {
        DevBuf parent, comp, same_deg, is_node, collides, fam_off, fam_of_label, run_off, run_of;
        DevBuf mk_a, mk_b, mv_a, mv_b;              // F-members: (label, gene) sort
        DevBuf ck_a, ck_b, cv_a, cv_b;              // F-collide: by genome, then by label
        DevBuf ek_a, ek_b, ev_a, ev_b;              // a caller's edges: intra-genome (lo, hi) keys and the sort's unused values
        DevBuf up_src, up_dst, up_gen;              // a caller's edges and genome ids on the device
        EventSpans<2> spans;                        // the id check and the rest (one stretch when nothing is checked)
    } fb;
    bool fam_valid = false;
    pdl_fam_result fam;
    uint64_t fam_serial = 0;          // counts the runs of K-fam over the context's own edges: what pb's copy of c->fam is checked against
    // K-place (pdl_place.h): the context's own families on the device (uploaded once per K-fam run: fb's buffers are work buffers that
    // pdl_families_of_edges overwrites), a caller's base, and the work buffers of one placement
    struct PlaceBufs {
        BaseBufs base;                              // the context's own
        uint64_t base_serial = 0;                   // c->fam_serial the copy was made at (0: none)
        BaseBufs up;                                // a caller's base ...
        DevBuf up_gen, up_src, up_dst;              // ... its genome ids and the caller's edges
        DevBuf ctl;                                 // u64 [PDL_PL_WORDS]
        DevBuf bctl, blay, up_edge_begin, up_n_query;   // a batch: u64 [PDL_PB_WORDS]; the queries' layout; the callers' lists'
        QSpans bspans;                              // ... and the stretch of device work of a chunk's K-bbh
        BbhBufs bbh;                                // K-bbh over the query block or the chunk: K-place's own set, never the context's
        DevBuf parent, is_node, same_deg, family_of, gcol, grp_of_label, gq_off, gb_off, group_base, mpre;
        DevBuf mk_a, mk_b, mv_a, mv_b;              // (root, query gene) sort
        DevBuf bk_a, bk_b, bv_a, bv_b, uniq;        // (group, base component) keys; then (group, genome) keys of the bridged members
        DevBuf ek_a, ek_b, ev_a, ev_b;              // a caller's edges: query-query (lo, hi) keys
        QSpans spans;                               // up to three stretches of device work
    } pb;
    // K-split (pdl_split.h): the packed graphs of one chunk on the device, its workgroups' scratch, and the timer of the launches
    struct SplitBufs {
        DevBuf desc, adj_off, adj, eid, ends, slots, out_edge, out_count, scratch;
        EventSpans<1> spans;
    } sb;
    uint64_t opt_split_scratch_bytes = 1ull << 30;  // pdl_split_first_level: scratch one launch may take
    // Pan-genome profile (pdl_profile.h): a caller's labelling and its sorted keys, the runs, the histograms; a caller's profile
    // and orders, the presence bits, the orders' histograms and curves.  Work buffers of one call, grown as needed.
    struct ProfileBufs {
        DevBuf ctl;                                 // u64 [PDL_PF_WORDS]
        DevBuf up_fam, up_gen, k_a, k_b, v_a, v_b;  // (label, genome) keys and the sort's values
        DevBuf inc_start, inc_genome, inc_label, inc_of_pos, fam_start, label, genome_off, fam_of_label, size, spread, copies, size_hist, hist;
        DevBuf up_orders, up_off, up_genomes, bits, order_hist, pan, core;
        EventSpans<2> spans;                        // the check and the rest
    } pf;
    // Genome-by-genome shared-family matrices (pdl_matrix.h): a caller's profile, the families' extra bit columns and where they
    // start, one slab of the genomes' bit rows, the two matrices.  Work buffers of one call, grown as needed.
    struct MatrixBufs {
        DevBuf ctl;                                 // u64 [PDL_MX_WORDS]
        DevBuf up_off, up_genomes, up_copies, extra, extra_off, bits, shared, shared_copies;
        EventSpans<1> spans;
    } mx;
    uint64_t opt_matrix_slab_bytes = 1ull << 28;    // pdl_genome_matrix: bytes the bit rows of one slab may take
    EventSpans<2> set_spans;         // pdl_append_genomes, pdl_remove_genomes (they exclude each other): the call's two stretches of device work
    // pdl_remove_genomes (pdl_remove.h): work buffers — until the host has read `ctl` the context itself is only read
    struct RemoveBufs {
        DevBuf gmap;                  // u32 [G] new genome id, RM_GONE for a genome that leaves
        DevBuf gen_in;                // u32 [N] genome ids, when the context's copy on the device is a caller's buffer that may be gone
        DevBuf new_id;                // u32 [N] new gene id, RM_GONE for a gene that leaves
        DevBuf kseq, gen, glen;       // u32 [N'] compacted kseq_len / genome ids / gene_len: they swap places with the context's
        DevBuf tile;                  // u32 [tiles] k-mers that stay per tile of the stream, then their exclusive scan
        DevBuf ctl;                   // u64 [PDL_RM_WORDS]
    } rm;
    uint8_t alpha_present[256] = {};  // letters of the base (residue histogram > 0): what a query may contain
    // K-rekey (pdl_rekey.h): option "alphabet_rekey" — an append or a removal that changes the alphabet writes the stream's keys again
    bool opt_alphabet_rekey = false;
    bool short_valid = false;                 // h_short_letters describes the set (built with the option on, kept up by appends and removals)
    std::vector<uint32_t> h_short_letters;    // [G][8] 256 bits per genome: the letters of its genes shorter than k (they show in no key)
    struct RekeyBufs {
        DevBuf keys;                          // the re-keyed stream on its way into keys_b (then: the old keys, released behind the call)
        DevBuf table, short_letters;          // K-rekey's table on the device; k_short_letters' output
        std::vector<uint64_t> h_table;        // (kept alive for the asynchronous upload)
        std::vector<uint32_t> h_table32;
    } rk;
    pdl_rekey_info last_rekey{};              // what the last append or removal did (pdl_get_rekey_info)

    pdl_timings tm{};
    EventPair ev[17];
    uint8_t *pin = nullptr;       // pinned host scratch for the small device->host reads (true async DMA, no staging copy)
    uint8_t *pin_dev = nullptr;   // the same buffer as the device addresses it (hipHostGetDevicePointer)
    size_t pin_bytes = 0;
    uint32_t pin_epoch = 0;       // last value a k_pin_read raised the flag at the tail of `pin` to
    // host mirror of the whole scoring result (pinned): filled by ONE set of device->host copies at the first
    // pdl_compute_scores after a scoring pass, so the per-genome calls are host memcpys (results up to PDL_MIRROR_LIMIT)
    uint8_t *mirror = nullptr;
    size_t mirror_bytes = 0;
    bool mirror_valid = false;
};

#include "pdl_state.h"        // the reset and the gate over the state words above

// The one place where exceptions become return codes: runs an entry point's body (-> its return code); what the body throws is
// translated and the message stored in the context (pdl_create's, through pdl_set_create_error, when there is none), after `undo`
// has freed and zeroed the outputs a failure must not leave behind.  The caller holds the context's lock — or, with Lock::take,
// has let go of it and the message is stored under it.
void pdl_set_create_error(const std::string &msg);
enum class Lock { held, take };
template <class Body, class Undo>
inline int guarded(pdl_ctx *c, Lock lock, Body &&body, Undo &&undo) {
    int code = PDL_ERR_DEVICE;
    std::string msg;
    try { return body(); }
    catch (const pdl_error &e) { code = e.code; msg = e.msg; }
    catch (const std::bad_alloc &) { msg = "host allocation failed"; }
    catch (const std::exception &e) { msg = e.what(); }
    undo();
    if (!c) pdl_set_create_error(msg);
    else if (lock == Lock::take) { std::lock_guard<std::mutex> lk(c->mu); c->err = msg; }
    else c->err = msg;
    return code;
}
template <class Body> inline int guarded(pdl_ctx *c, Body &&body) { return guarded(c, Lock::held, body, [] {}); }

// Small device->host reads through the pinned scratch: queue with add(), one sync(), then read the returned pointers.
// Small device -> host reads (counters, control blocks) WITHOUT a DMA copy and without hipStreamSynchronize: on this
// platform a copy of a few hundred bytes is ~30 us of copy-engine latency and the wake-up from a stream wait another
// 20-30 — and a step of the 64-genome set has three such reads.  Instead one tiny kernel, stream-ordered behind the work
// it reads, stores the words straight into pinned host memory (PCIe posted writes), fences at system scope and raises an
// epoch flag in the same buffer; the host spins on the flag (a few us).  A read that is large, oddly sized or does not
// fit the pinned buffer, and a wait that outlasts the spin budget (the stream has long kernels ahead), take the old road.
struct PinReadArgs {
    const uint32_t *src[8];
    uint32_t dst_word[8], words[8];
    uint32_t n;
    uint32_t *pin;             // pinned host buffer as the device sees it
    uint32_t flag_word, epoch;
};
// The arrival checksum weights every word by its position in the WHOLE pinned buffer (odd weights: a single late word always
// shows) — weights that restarted in every segment let two late words at the same index of different segments cancel.
__host__ __device__ inline uint32_t pin_weight(uint32_t dst_word) { return 2u * dst_word + 1u; }
// Host side of the protocol, on plain memory (exported for the CPU tests as pdl_pin_arrived): the flag shows this read's epoch
// AND the words in place add up to the checksum the kernel left beside the flag.
inline bool pin_arrived(const volatile uint32_t *pin, const uint32_t *dst_word, const uint32_t *words, uint32_t n, uint32_t flag_word, uint32_t epoch) {
    if (pin[flag_word] != epoch) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    uint32_t sum = 0;
    for (uint32_t s = 0; s < n; s++)
        for (uint32_t i = 0; i < words[s]; i++) sum += pin[dst_word[s] + i] * pin_weight(dst_word[s] + i);
    return sum == pin[flag_word + 1];
}
#ifdef __HIPCC__
static __global__ __launch_bounds__(256) void k_pin_read(PinReadArgs a) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    pdl_sync();
    uint32_t sum = 0;
    for (uint32_t s = 0; s < a.n; s++)
        for (uint32_t i = threadIdx.x; i < a.words[s]; i += 256) { const uint32_t v = a.src[s][i]; a.pin[a.dst_word[s] + i] = v; sum += v * pin_weight(a.dst_word[s] + i); }
    atomicAdd(&s_sum, sum);
    __threadfence_system();
    pdl_sync();
    // The flag says "all of it has been sent", the checksum beside it lets the host see that all of it has ARRIVED: the
    // words travel from several waves over several paths, and the flag may overtake the last of them.
    if (threadIdx.x == 0) {
        *(volatile uint32_t *) (a.pin + a.flag_word + 1) = s_sum;
        __threadfence_system();
        *(volatile uint32_t *) (a.pin + a.flag_word) = a.epoch;
        __threadfence_system();
    }
}
#endif
constexpr size_t PDL_PIN_FLAG_BYTES = 64;                    // the tail of the pinned buffer holds the flag
struct PinRead {
    pdl_ctx *c;
    size_t used = 0;
    PinReadArgs k{};
    bool by_copy = false;                                    // at least one read went through hipMemcpyAsync
    std::vector<std::pair<void *, std::pair<const void *, size_t>>> spill;   // reads that did not fit: done pageable
    explicit PinRead(pdl_ctx *ctx) : c(ctx) {}
    template <class T> const T *add(const void *d_src, size_t count) {
        const size_t bytes = count * sizeof(T);
        const size_t at = (used + 15) & ~(size_t) 15;
        const size_t room = c->pin_bytes > PDL_PIN_FLAG_BYTES ? c->pin_bytes - PDL_PIN_FLAG_BYTES : 0;
        if (c->pin && at + bytes <= room) {
            used = at + bytes;
            if (k.n < 8 && bytes % 4 == 0 && bytes <= (64u << 10) && (reinterpret_cast<uintptr_t>(d_src) & 3) == 0) {
                k.src[k.n] = static_cast<const uint32_t *>(d_src); k.dst_word[k.n] = (uint32_t) (at / 4); k.words[k.n] = (uint32_t) (bytes / 4);
                k.n++;
            } else {
                by_copy = true;
                PDL_HIP(hipMemcpyAsync(c->pin + at, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
            }
            return reinterpret_cast<const T *>(c->pin + at);
        }
        void *h = malloc(bytes ? bytes : 1);
        spill.push_back({h, {d_src, bytes}});
        by_copy = true;
        PDL_HIP(hipMemcpyAsync(h, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        return reinterpret_cast<const T *>(h);
    }
    bool issued = false;
    void issue() {                                           // queue the read now; the host may do other work before wait()
        if (issued) return;
        issued = true;
        if (!k.n) return;
        k.pin = reinterpret_cast<uint32_t *>(c->pin_dev ? c->pin_dev : c->pin);     // (the buffer as the device addresses it)
        k.flag_word = (uint32_t) ((c->pin_bytes - PDL_PIN_FLAG_BYTES) / 4);
        k.epoch = ++c->pin_epoch;
        hipLaunchKernelGGL(k_pin_read, dim3(1), dim3(256), 0, c->stream, k);
        PDL_HIP(hipGetLastError());
    }
    void sync() {
        issue();
        if (k.n) {
            if (!by_copy) {
                const volatile uint32_t *words = reinterpret_cast<const volatile uint32_t *>(c->pin);
                auto arrived = [&]() -> bool { return pin_arrived(words, k.dst_word, k.words, k.n, k.flag_word, k.epoch); };    // flag up and every word in place
                const auto t0 = std::chrono::steady_clock::now();
                bool ok = false;
                for (uint32_t spins = 0; !(ok = arrived()); spins++) {
                    if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
                    __builtin_ia32_pause();
                }
                if (ok) { std::atomic_thread_fence(std::memory_order_acquire); return; }
            }
        }
        PDL_HIP(hipStreamSynchronize(c->stream));
    }
    ~PinRead() { for (auto &e : spill) free(e.first); }
};
// A counted gate: what a checking kernel left at d_word comes to the host in a read of its own; the caller words the refusal.
// With `spans`: the stretch of device work it has open ends in front of the read and the next one opens behind it.
inline uint64_t pdl_gate(pdl_ctx *c, const uint64_t *d_word) {
    PDL_HIP(hipGetLastError());
    PinRead rd(c);
    const uint64_t *w = rd.add<uint64_t>(d_word, 1);
    rd.sync();
    return *w;
}
template <class Spans> inline uint64_t pdl_gate(pdl_ctx *c, Spans &spans, const uint64_t *d_word) {
    spans.end();
    const uint64_t v = pdl_gate(c, d_word);
    spans.begin();
    return v;
}
// the control block of a context that has built nothing yet: the sort's word (and K-fam's) is all a call on it needs
inline void pdl_ctl_ready(pdl_ctx *c) { if (!c->scalars.p) c->scalars.alloc((PDL_CTL_LAST + 1) * sizeof(uint64_t)); }

// stage entry points (pdl_dict.hip / pdl_join.hip)
void pdl_run_preprocess(pdl_ctx *c, int kvalue, bool only_complexity);
void pdl_run_reshard(pdl_ctx *c);       // the range lists again, for the genomes of c->shard, on the dictionary that is there
void pdl_run_dist_begin(pdl_ctx *c, int kvalue);
void pdl_run_dist_finish(pdl_ctx *c, uint64_t total_records, const uint64_t *genome_weights);
bool pdl_run_dist_ranges(pdl_ctx *c, const uint64_t *run_records, const uint64_t *genome_weights, const uint64_t *genome_costs);   // false: not available for this build (use pdl_run_dist_finish)
void pdl_run_dist_finish_ranges(pdl_ctx *c, uint64_t total_records, uint32_t *d_keys, unsigned long long *d_ranges, uint64_t n_tuples, const uint64_t *counter_sums);
void pdl_run_score_all(pdl_ctx *c);
void pdl_run_dist_score_begin(pdl_ctx *c);
void pdl_run_dist_score_finish(pdl_ctx *c, const pdl_dist_cell *d_inbox, uint64_t n_inbox);
void pdl_prepare_tasks(pdl_ctx *c);
void pdl_run_bbh_all(pdl_ctx *c);
// K-fam (pdl_families.h, pdl_bbh.hip): components, members and collision flags from up to two device edge lists
void pdl_run_families(pdl_ctx *c, const int32_t *const src[2], const int32_t *const dst[2], const uint64_t n_edges[2], bool mirrored0, bool check_ids,
                      bool dedupe_intra, const uint32_t *d_gen, uint32_t N, uint32_t genome_bits, pdl_fam_result &out);
void pdl_run_families_of_context(pdl_ctx *c);       // ... over the context's own edges (K-bbh has run) -> c->fam
// K-split (pdl_split.h, pdl_bbh.hip): the first level of Girvan-Newman on every graph of a packed batch; pdl_split without the C allocation
struct pdl_split_result {
    uint32_t graphs = 0, chunks = 0;
    uint64_t nodes = 0, edges = 0, rounds = 0;
    std::vector<uint64_t> removed_off;
    std::vector<uint32_t> removed_u, removed_v;
    float device_ms = 0.f;
};
void pdl_run_split(pdl_ctx *c, uint32_t n_graphs, const uint64_t *node_off, const uint64_t *adj_off, const uint32_t *adj, pdl_split_result &out);
// Pan-genome profile (pdl_profile.h, pdl_bbh.hip): pdl_profile and pdl_curves without the C allocation.  hist: spread_hist [G + 1] |
// spread_by_genome [(G + 1) * G] | the genomes' genes [G] | ... in core, accessory, unique families [3][G]
struct pdl_profile_result {
    uint32_t n_sequences = 0, n_genomes = 0, families = 0, incidences = 0, max_size = 0, core = 0, single_copy_core = 0, unique = 0, accessory = 0;
    std::vector<uint32_t> label, size, spread, genome_off, genomes, copies, size_hist, hist;
    float device_ms = 0.f;
};
struct pdl_curves_result {
    uint32_t n_genomes = 0, n_orders = 0, families = 0, incidences = 0;
    std::vector<uint32_t> pan, core;
    float device_ms = 0.f;
};
void pdl_run_profile(pdl_ctx *c, const uint32_t *family_of, const uint32_t *genome_of, uint32_t N, uint32_t G, pdl_profile_result &out);
void pdl_run_pan_curves(pdl_ctx *c, const pdl_profile *profile, const uint32_t *orders, uint32_t n_orders, pdl_curves_result &out);
// Genome-by-genome shared-family matrices (pdl_matrix.h, pdl_bbh.hip): pdl_genome_matrix's struct without the C allocation
struct pdl_matrix_result {
    uint32_t n_genomes = 0, families = 0, incidences = 0, levels = 0, slabs = 0, splits = 0;
    std::vector<uint32_t> shared, shared_copies;
    float device_ms = 0.f;
};
void pdl_run_genome_matrix(pdl_ctx *c, const pdl_profile *profile, pdl_matrix_result &out);
void pdl_ensure_costs(pdl_ctx *c);
void pdl_input_arrived(pdl_ctx *c);      // deferred device input: waits for the genome ids / offset ends and checks them
void pdl_finish_layout(pdl_ctx *c);      // ... then builds the genome layout on the host
// K-query (pdl_query.h): K-rank + K-sort + K-rle of the query genes with the base's rank parameters (pdl_dict.hip); the records
// land in (recpos, post), their count at d_u; returns the buffer that holds the sorted keys
const void *pdl_query_dictionary(pdl_ctx *c, const uint8_t *res, const uint64_t *off, const uint64_t *kmer_off, uint32_t n, uint64_t m,
                                 uint64_t n_res, void *keys_a, void *keys_b, uint32_t *vals_a, uint32_t *vals_b, uint32_t *recpos, uint2 *post,
                                 uint64_t *d_u);
// ... with another alphabet's rank table and key width than the context's (option "query_rekey": the union's)
const void *pdl_query_dictionary(pdl_ctx *c, const RankParams &rp, bool key64, const uint8_t *res, const uint64_t *off, const uint64_t *kmer_off,
                                 uint32_t n, uint64_t m, uint64_t n_res, void *keys_a, void *keys_b, uint32_t *vals_a, uint32_t *vals_b,
                                 uint32_t *recpos, uint2 *post, uint64_t *d_u);
// Option "query_rekey" (pdl_rekey.h, pdl_dict.hip).  The alphabet decision for the letters (256 bits) queries bring on top of the
// base's: false when the union's ranks would not be exact (*why: rk_why_not), else the union's table and the plans are in
// c->qb.rk when `adopt` is set, their tables on their way to the device.  pdl_query_rebase queues, for the plan in c->qb.rk, the
// fold's three base ranks in the union's alphabet (up3) and Q-rebase over the query records: record j's key is qkeys[recpos[j]]
// (recpos NULL: qkeys[j]), j below *d_records and below `bound`.
bool pdl_query_rekey_base_exact(const pdl_ctx *c, const char **why);
bool pdl_query_rekey_plan(pdl_ctx *c, const uint32_t letters[8], bool adopt, const char **why);
void pdl_query_rebase(pdl_ctx *c, const void *qkeys, const uint32_t *recpos, const unsigned long long *d_records, uint64_t bound);
void pdl_run_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n, pdl_scores *out, pdl_query_info *info);
// ... its device half alone: everything up to the ordered cells, which stay in HBM (K-place filters them there)
pdl_query_cells pdl_run_query_device(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n);
// K-place (pdl_place.h, pdl_bbh.hip): the query's edges (K-bbh over the query block) and their placement on the context's families;
// the placement of a caller's edge list (device pointers, union ids) on a base
void pdl_run_place_query(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, uint32_t n, pdl_place_result &out, pdl_query_info *info);
// a base's families (the context's own or a caller's, checked) on their way to the device, into `b` -> the device view
PlaceBase pdl_upload_base(pdl_ctx *c, const FamView &f, BaseBufs &b, const uint32_t *d_genome_of, uint32_t G);
void pdl_run_place_edges(pdl_ctx *c, const PlaceBase &base, uint32_t n_query, const int32_t *d_src, const int32_t *d_dst, uint64_t n_edges,
                         pdl_place_result &out);
// K-query for a batch (pdl_query_batch.h): q genomes, each scored on its own; gene_begin [n_queries + 1] cuts the n genes
void pdl_run_query_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                         pdl_scores *out, pdl_query_info *info, pdl_query_batch_info *binfo);
// ... its plan (the domain refusals, every query's sizes and weight — column_bytes more per column of its union; -> the HBM tables'
// columns), its chunking rule and the device
// half of one chunk [qa, qe): everything up to the ordered cells, which stay in HBM (K-place for a batch filters them there)
uint32_t pdl_query_batch_plan(pdl_ctx *c, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries, std::vector<QBQuery> &qs,
                              uint64_t column_bytes);
uint32_t pdl_query_batch_chunk_end(const pdl_ctx *c, const std::vector<QBQuery> &qs, uint32_t qa);
pdl_query_cells pdl_run_query_chunk_device(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const std::vector<QBQuery> &qs, uint32_t qa, uint32_t qe,
                                           uint32_t hbm_cols);
// K-place for a batch (pdl_place_batch.h, pdl_bbh.hip): out [n_queries]; info [n_queries] or NULL
void pdl_run_place_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                         std::vector<pdl_place_result> &out, pdl_query_info *info, uint32_t *chunks, float *device_ms);
// ... and of callers' lists on a caller's base: n_query [n_queries], edge_begin [n_queries + 1] from 0, the lists end to end on the device
void pdl_run_place_batch_edges(pdl_ctx *c, const PlaceBase &base, uint32_t n_queries, const uint32_t *n_query, const uint64_t *edge_begin,
                               const int32_t *d_src, const int32_t *d_dst, std::vector<pdl_place_result> &out);
void pdl_check_alphabet(pdl_ctx *c, const uint8_t *d_res, uint64_t n, unsigned long long *d_bad);      // k_q_absent over device bytes (pdl_query.h)
[[noreturn]] void pdl_fail_absent_byte(uint64_t bad_word, const char *who);                             // ... and the refusal that names the byte
// K-append (pdl_append.h, pdl_dict.hip): the n genes of residues/offsets become genes N.. of the context; genome_ids [n] are their
// union genome ids (checked by the caller), n_new_genomes of them new.  pdl_extend_layout (pdl_api.hip): the host's genome layout.
void pdl_run_append(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *genome_ids, uint32_t n, uint32_t n_new_genomes,
                    pdl_append_info *info);
void pdl_extend_layout(pdl_ctx *c, const uint32_t *genome_ids, uint32_t n);
// K-remove (pdl_remove.h, pdl_dict.hip): the genes of the `count` listed genomes (distinct ids < G, not all of them: checked by the
// caller) leave the context.  pdl_replace_layout (pdl_api.hip): the host's genome layout for the genes that stay.
void pdl_run_remove(pdl_ctx *c, const uint32_t *genomes, uint32_t count, pdl_remove_info *info);
void pdl_replace_layout(pdl_ctx *c, std::vector<uint32_t> &&genome_of);
inline uint2 *pdl_postings(const pdl_ctx *c) { return c->post_ext ? c->post_ext : c->post.as<uint2>(); }

// compute units of the context's device (looked up once; 256 where the runtime does not say)
inline int pdl_cus(pdl_ctx *c) {
    if (c->cus <= 0) {
        hipDeviceProp_t prop;
        c->cus = hipGetDeviceProperties(&prop, c->device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    return c->cus;
}

// event helpers
enum { EV_HIST, EV_RANK, EV_SORT1, EV_DICT, EV_SORT2, EV_RANGES, EV_JOIN, EV_JOIN_OVF, EV_ORDER, EV_PRE_TOTAL, EV_SCORE_TOTAL,
       EV_DIST_BEGIN, EV_DIST_FINISH, EV_DIST_SCORE_FINISH, EV_DIST_RANGES, EV_MERGE, EV_REKEY, EV_COUNT };
static_assert(EV_COUNT <= 17, "pdl_ctx::ev");

// An event record is a marker packet between two dispatches (a few us of idle stream each); the per-stage pairs can be
// switched off ("stage_timers" 0) when only the totals and the join's launch time are wanted (bench.py's timed loop).
inline bool ev_is_stage(int i) { return i == EV_HIST || i == EV_RANK || i == EV_SORT1 || i == EV_DICT || i == EV_SORT2 || i == EV_RANGES || i == EV_ORDER || i == EV_JOIN_OVF || i == EV_MERGE || i == EV_REKEY; }
inline void ev_begin(pdl_ctx *c, int i) {
    c->ev[i].used = false;
    if (!c->opt_stage_timers && ev_is_stage(i)) return;
    if (!c->ev[i].a) { PDL_HIP(hipEventCreate(&c->ev[i].a)); PDL_HIP(hipEventCreate(&c->ev[i].b)); }
    PDL_HIP(hipEventRecord(c->ev[i].a, c->stream));
}
inline void ev_end(pdl_ctx *c, int i) {
    if (!c->opt_stage_timers && ev_is_stage(i)) return;
    PDL_HIP(hipEventRecord(c->ev[i].b, c->stream));
    c->ev[i].used = true;
}
inline float ev_ms(pdl_ctx *c, int i) {
    if (!c->ev[i].used) return 0.f;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[i].a, c->ev[i].b) != hipSuccess) return 0.f;
    return ms;
}

// Genes that are not the context's input (a query, an append), as the host lays them out for K-rank from the caller's offsets:
// residues from 0, k-mer offsets, k-mer counts.  The limits on R and M are the caller's (a query's differ from an append's).
struct NewGenes {
    std::vector<uint64_t> off, koff;        // [n + 1] residue / k-mer offset of every gene
    std::vector<uint32_t> kseq, len;        // [n] k-mers / residues of every gene (a gene of 2^32 residues and more: 0xffffffff; the callers' limits exclude it)
    uint64_t r0 = 0, R = 0, M = 0;          // the caller's first residue; residues; k-mers
    NewGenes(const uint64_t *offsets, uint32_t n, uint32_t k) : off(n + 1), koff(n + 1), kseq(n), len(n) {
        r0 = offsets[0]; R = offsets[n] - r0;
        for (uint32_t g = 0; g < n; g++) {
            const uint64_t l = offsets[g + 1] - offsets[g];
            len[g] = (uint32_t) std::min<uint64_t>(l, 0xffffffffull);
            off[g] = offsets[g] - r0;
            koff[g] = M;
            kseq[g] = l >= k ? (uint32_t) std::min<uint64_t>(l - k + 1, 0xffffffffull) : 0u;
            M += kseq[g];
        }
        off[n] = R; koff[n] = M;
    }
    // ... on their way into c->qb (res with 16 bytes of slack, off, koff, kseq), queued on the context's stream
    void upload(pdl_ctx *c, const uint8_t *residues) const {
        auto &q = c->qb;
        hipStream_t st = c->stream;
        const size_t n = kseq.size();
        q.res.alloc(R + 16); q.off.alloc((n + 1) * 8); q.koff.alloc((n + 1) * 8); q.kseq.alloc(n * 4);
        if (R) PDL_HIP(hipMemcpyAsync(q.res.p, residues + r0, R, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(q.off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(q.koff.p, koff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        PDL_HIP(hipMemcpyAsync(q.kseq.p, kseq.data(), n * 4, hipMemcpyHostToDevice, st));
    }
};

static inline uint32_t bit_length64(uint64_t v) {
    uint32_t b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}
