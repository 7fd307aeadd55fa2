// pdl_join.hip — the scoring stage on the device: computeScores (ig/native/library.cpp:409-527) for
// every gene (row) of every genome of the shard in one pass.
//
//   K-join      k_join_lds<HT, T, FILTER>   sparse all-vs-all multiset-Jaccard join of one row against the
//                            dictionary, accumulators in an LDS hash table (the reference's dense N-length arrays
//                            + colour stamps, library.cpp:421-426,467-477), fused finalize (library.cpp:493-517)
//                            and per-(row, genome) / per-column maxima.  Tier 1 = small table behind a
//                            "seen twice" bitmap filter (several rows per CU), tier 2 = 8192-slot table
//   K-join-hbm  k_join_hbm   tier 3: same row program with direct-addressed tables in HBM
//   K-order     k_mirror_cells_sub, k_order_rows_sub  every row's cells in the reference's emission order
//                            (first-touch order, library.cpp:456-482,493 — SURVEY.md §8a row 9a)
//
// Row program (all tiers).  A row gene r owns a list of posting ranges, one per record of r that sits in a
// rank-group of >= 2 records: {first posting, postings, own count, group size}.  For every posting
// {c, cnt_c} of every range with own count cnt_r (library.cpp:461-479):
//       inter[c] += min(cnt_c, cnt_r);  perc_cnt[c] += cnt_r;  tr_cnt[c] += cnt_c
// The three sums are packed in one 64-bit word (21 bits each: every sum is bounded by twice the k-mer count
// of a gene, and genes with >= 2^20 k-mers are refused up front), so one update is one 64-bit LDS atomic.
// `first` keeps the smallest group start that touched c: the reference emits a row's cells by (column chunk
// of 2048, first range that touched the column, column), and group starts are monotone in the row's range order.
//
// Mirror mode (whole dataset on one device).  Cell (c, r) holds the sums of cell (r, c) with perc_cnt and
// tr_cnt swapped, and the reference computes both.  Groups are gene-sorted, so a row's ranges start right
// after its own record: a row only meets the genes above it, and every staged cell also stands for its
// transpose, which K-order hands to the column's row.  With a genome shard (multi-GPU) rows keep whole groups.
#include "pdl_common.h"
#include "pdl_scan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

constexpr int HBM_THREADS = 512;                      // workgroup of the HBM-table kernel
constexpr uint32_t EMPTY_KEY = 0xffffffffu;
constexpr uint64_t FIELD_MASK = (1ull << 21) - 1;
constexpr uint32_t CELL_CHUNK = 16384;                 // staging cells a workgroup reserves at a time (>= any row's candidates in LDS)

struct JoinArgs {
    const uint2 *post;
    const uint4 *ranges;           // {first posting, postings, own count, group size} per range, or ...
    const uint2 *ranges8;          // ... (non-null) packed: {first posting, postings | min(own count, 1023) << 22}; the range sits right behind
                                   //     its own record, so a count of 1023 or more is read from there; the group is named by its END
    const uint32_t *seq_off;
    const uint32_t *kseq_len;
    const uint32_t *genome_of;
    const uint4 *gene_info;        // per gene {k-mers, genome, task position (0xffffffff: not this context's row), shard-local index of its genome}:
                                   // what finalize wants to know about a column, in ONE dependent load instead of four
    const uint32_t *task_rows;     // gene id of task position p
    const uint32_t *task_lg;       // shard-local genome of task position p
    const uint32_t *work;          // task positions to process (k_join_hbm: the overflow list)
    const uint4 *desc;             // k_join_lds: {task position, gene, first range, ranges} per work item
    uint32_t n_work;
    const uint32_t *n_work_ptr;    // when set: number of work items, produced on the device by the previous tier
    uint32_t N, G, k;
    uint32_t min_kseq;             // smallest non-zero kseq_length of the dataset (finalize pre-filter)
    uint32_t canonical;            // PDL_FLAG_CANONICAL_ORDER: no first-touch tracking
    float *MS;                     // [n_task_rows][G]
    float *CM;                     // [shard][N]
    uint32_t *row_base, *row_cnt;  // [n_task_rows]
    float *st_score, *st_perc, *st_tr;
    uint32_t *st_col, *st_first;
    uint32_t mirror;               // 1: ranges hold only columns above the row; every cell (r,c) also stands for (c,r)
    const uint32_t *taskpos_of;    // mirror mode: task position of every gene (0xffffffff: the gene is another GPU's row)
    const uint32_t *local_genome;  // mirror mode: index of every genome in this context's shard (CM row)
    uint32_t *mirror_cnt;          // mirror mode: mirrored cells per task position
    unsigned long long st_cap;
    uint32_t *work_cursor;         // persistent-workgroup row dispenser (one atomic hands out `work_batch` items:
                                   // a single device-scope word serves only ~90 dequeues/us)
    uint32_t work_batch;
    uint32_t sift_threshold;       // tier 0: 1 = the sift asks of a column what finalize will ask of it, 0 = two sightings (pdl_set_option "sift_threshold")
    unsigned long long *cell_cursor;
    uint32_t *overflow_count;
    uint32_t *error_count;         // internal consistency violations (must stay 0)
    uint32_t *overflow_rows;
    uint4 *overflow_desc;          // (LDS tiers) the handed-on rows' descriptors, written beside their task positions: the next tier starts without a pass that makes them
#ifdef PDL_JOIN_PHASES
    unsigned long long *phase;     // diagnostic build (-DPDL_JOIN_PHASES): time the first thread of every workgroup spends in the phases of a row (100-MHz ticks, summed)
#endif
    void *defer;                   // filter tiers: per workgroup, the first light sightings of the row in hand: {column | tag << 22, 0xffffffff - group key}
                                   // (8 bytes, gene ids below 2^22) or {column, 0xffffffff - group key, row, launch} (16 bytes), see defer_wide
    uint32_t defer_wide;
    uint32_t defer_cap;            // entries per workgroup; a row with more goes to the next tier
    uint32_t *reload_count;        // entries that were not there at the first look (diagnostic, pdl_timings.aside_reloads)
    uint32_t defer_serial;         // this launch's number: with the row it makes an entry recognisable as written for THIS row
    // HBM tables (k_join_hbm only): per workgroup acc u64[N], first u32[N], touched u32[N], emit u32[N]
    unsigned long long *hbm_acc;
    uint32_t *hbm_u32;
};

// smallest integer n with (float) n / denom >= threshold (the quotient is monotone in n; n < 2^24 is exact in float)
__host__ __device__ __forceinline__ uint32_t min_numerator(float threshold, float denom) {
    uint32_t n = (uint32_t) (threshold * denom);
    n = n > 2 ? n - 2 : 0;
    while ((float) (int) n / denom < threshold) n++;
    return n;
}

// finalize one candidate (library.cpp:494-502); returns score (0 when not emitted)
__device__ __forceinline__ float finalize_counts(int inter, int pc, int tc, uint32_t my_kcnt, uint32_t other_kcnt, float threshold,
                                                 float &perc, float &tr_perc) {
    const int union_size = (int) my_kcnt + (int) other_kcnt - inter;
    perc = (float) pc / (float) (int) my_kcnt;
    tr_perc = (float) tc / (float) (int) other_kcnt;
    const bool score_valid = perc >= threshold || tr_perc >= threshold;
    return (float) inter / (float) union_size * (score_valid ? 1.0f : 0.0f);
}
__device__ __forceinline__ float finalize_cell(unsigned long long acc, uint32_t my_kcnt, uint32_t other_kcnt, float threshold,
                                               float &perc, float &tr_perc) {
    const int inter = (int) (acc & FIELD_MASK);
    const int pc = (int) ((acc >> 21) & FIELD_MASK);
    const int tc = (int) (acc >> 42);
    const int union_size = (int) my_kcnt + (int) other_kcnt - inter;
    perc = (float) pc / (float) (int) my_kcnt;
    tr_perc = (float) tc / (float) (int) other_kcnt;
    const bool score_valid = perc >= threshold || tr_perc >= threshold;
    return (float) inter / (float) union_size * (score_valid ? 1.0f : 0.0f);
}

#include "pdl_join_part.h"       // K-join, partition tier (short rows, several per workgroup cycle)

// ------------------------------------------------------------------------------------------------
// K-join (LDS table).  Persistent workgroups pull rows (work items) from a global cursor.
//
// Per row:
//   stage     the row's ranges are copied to LDS (coalesced 16-byte loads) with the exclusive prefix of
//             their lengths: the row's lookups become one flat index space [0, L)
//   lookups   lane t handles flat indices t, t+T, ...; four at a time: four binary searches in the LDS
//             prefix (independent, interleaved by the compiler), then four 8-byte posting loads in flight
//   finalize  touched slots only (the reference's colored_cells); candidates that cannot pass the
//             validity threshold are dropped before their column's k-mer count is fetched; cells are
//             written where they are decided, into a staging chunk owned by the workgroup
// The table is cleared once per workgroup; afterwards every slot is reset by whoever consumes it.
//
// Two flavours of the lookup phase:
//   FILTER = false  one pass: every posting is probed/inserted and added (1 LDS read + 1 64-bit LDS atomic).
//                   The table must hold every column that shares a k-mer with the row, so it is big
//                   (8192 slots, 1 workgroup per CU).
//   FILTER = true   "seen twice" filter.  A column that shares exactly ONE k-mer occurrence pair with the
//                   row (one lookup, both counts 1) has inter = perc_cnt = tr_cnt = 1 and is valid only if
//                   1/K_row >= thr or 1/K_col >= thr, i.e. K <= 2k (library.cpp:497-500).  When the row and
//                   every gene of the dataset have more than 2k k-mers such a column can never be emitted,
//                   and on k-mer-rich data these are ~95 % of all columns a row touches.  Pass 1 sets a bit
//                   per (hashed) column in a 64-Kbit LDS bitmap and inserts the column key only when its bit
//                   was already set (second sighting; hash collisions only add keys) or the lookup is heavy
//                   (a count >= 2); pass 2 re-walks the lookups and adds the contributions of the columns
//                   that have a key.  Sums of inserted columns are complete and exact; dropped columns are
//                   exactly the ones the reference would not emit.  The table shrinks ~20x, so 5-8
//                   workgroups (rows) are resident per CU instead of one.
// Rows whose keys do not fit are appended to an overflow list for the next tier.
// ------------------------------------------------------------------------------------------------

// loads served by L2, never by L1 (agent scope = `sc1`): tables and lists in HBM that a workgroup writes (plain stores or
// L2 atomics) and reads back
__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 16-byte loads that L1 never serves (`sc1`: straight to this XCD's L2) — for data this CU has just rewritten
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ld16_sc1(const uint4 *p) {
    u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ void ld16_sc1_x4(const uint4 *const (&p)[4], u32x4 (&v)[4]) {
    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\t"
                 "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]) : "memory");
}

template <int HT_BITS_, int T_, bool FILTER>
struct JoinCfg {
    static constexpr uint32_t HT = 1u << HT_BITS_;
    static constexpr uint32_t LIMIT = HT - T_ - HT / 8;    // more keys than this: next tier
    static constexpr uint32_t TOUCH_CAP = LIMIT + T_;      // < HT: the probe loop always finds a free slot
    static constexpr uint32_t RPT = FILTER ? 2 : 1;        // ranges staged per thread and batch
    static constexpr uint32_t RB = RPT * T_;
    // "seen once" bitmap of the filter tier: 32 Kbit beside the 1024-slot table (keeps five workgroups per CU), 64 Kbit
    // beside the larger tables, whose rows hold far more lookups (a full bitmap filters nothing and overflows the table)
    static constexpr uint32_t BM_BITS_LOG2 = HT_BITS_ <= 10 ? 15 : 16;
    static constexpr uint32_t BM_WORDS = (1u << BM_BITS_LOG2) / 32;
    static_assert(TOUCH_CAP < HT, "table must never fill up");
    static_assert(TOUCH_CAP <= CELL_CHUNK, "a staging chunk must hold any row");
};

template <int HT_BITS_, int T_, bool FILTER>
__global__ __launch_bounds__(T_, (FILTER && HT_BITS_ <= 10) ? 5 : (FILTER && T_ == 256) ? 3 : 1) void k_join_lds(JoinArgs a) {
    using Cfg = JoinCfg<HT_BITS_, T_, FILTER>;
    constexpr uint32_t HT = Cfg::HT, LIMIT = Cfg::LIMIT, TOUCH_CAP = Cfg::TOUCH_CAP, RB = Cfg::RB, RPT = Cfg::RPT;
    constexpr int T = T_;
    // chunks of 64 lookups a wave has in flight per step.  Four beside the small table (95 VGPRs: five workgroups per CU); the
    // 2048-slot tier runs three workgroups per CU on LDS grounds and has registers to spare: eight chunks = twice the postings
    // in flight per wave, for rows whose time is the latency of those gathers (configs[4]: 31 k lookups per row)
    constexpr uint32_t NCH = (FILTER && HT_BITS_ == 11) ? 8 : 4;
    constexpr bool PROBE2 = FILTER && HT_BITS_ == 11;        // the table is probed two slots at a time
    __shared__ unsigned long long s_acc[HT];
    __shared__ uint2 s_kf[HT];                       // {column id, 0xffffffff - smallest group start that touched it}
    __shared__ uint32_t s_bm[FILTER ? Cfg::BM_WORDS : 1];
    __shared__ uint16_t s_touched[TOUCH_CAP];
    __shared__ uint2 s_gm[RB + 1];                   // staged ranges: {first posting, own count}
    __shared__ uint32_t s_gsv[RB + 1];               // and the start of their group (identifies the group: emission order)
    __shared__ uint32_t s_cum[RB + 66];               // exclusive prefix of their lengths, 0xffffffff beyond the batch
    __shared__ uint32_t s_wave[17];
    __shared__ uint2 s_wstart[T_ / PDL_WAVE];          // per wave: {range holding the first lookup of its segment, that range's start}
    __shared__ uint32_t s_ntouched, s_nemit, s_overflow, s_next, s_batch_end;
    __shared__ uint4 s_desc;
    __shared__ unsigned long long s_base, s_chunk_next, s_chunk_end;

    const uint32_t tid = threadIdx.x;
#ifdef PDL_JOIN_CHECK
    __shared__ uint32_t s_rowseq;
    uint32_t my_seq = 0;
#endif
    const uint32_t n_work = a.n_work_ptr ? *a.n_work_ptr : a.n_work;
    if (n_work == 0) return;                             // (uniform) a tier nobody handed a row to: leave before the table is cleared
    for (uint32_t i = tid; i < HT; i += T) { s_kf[i] = make_uint2(EMPTY_KEY, 0u); s_acc[i] = 0; }
    for (uint32_t i = RB + tid; i < RB + 66; i += T) s_cum[i] = 0xffffffffu;
    if (tid == 0) {
        s_gm[RB] = make_uint2(0u, 0u); s_gsv[RB] = 0u;
        s_ntouched = 0; s_nemit = 0; s_overflow = 0; s_chunk_next = 0; s_chunk_end = 0;
        const uint32_t w0 = atomicAdd(a.work_cursor, a.work_batch);
        s_next = w0; s_batch_end = w0 + a.work_batch;
        if (w0 < n_work) s_desc = a.desc[w0];
    }
    const float threshold = 1.0f / (2.0f * (float) a.k);
    const uint32_t tc_min = min_numerator(threshold, (float) (int) a.min_kseq);
    const bool track_first = a.canonical == 0;

#ifdef PDL_JOIN_PHASES
    unsigned long long ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t_prev = wall_clock64();
#define PH_MARK(i) do { if (tid == 0) { const unsigned long long t_now = wall_clock64(); ph[i] += t_now - t_prev; t_prev = t_now; } } while (0)
#define PH_WAIT() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define PH_MARK(i) do { } while (0)
#define PH_WAIT() do { } while (0)
#endif
    // insert column c if it has no slot yet; returns the slot (table can never be full, see TOUCH_CAP), NO_SLOT once the row has overflowed
    constexpr uint32_t NO_SLOT = 0xffffffffu;
    // claim the empty slot `slot` for column c: true = c sits there now (by this thread or by another one that was faster)
    auto claim = [&](uint32_t slot, uint32_t c, bool &give_up) -> bool {
        // a look at the key count on the (rare) insert path bounds the table: every thread that passes adds at most
        // one key before it looks again, so there are never more than LIMIT + T of them — and no lookup has to poll
        // the overflow flag (an LDS read per lookup, on a kernel whose LDS pipe is the busy one)
        if (*(volatile uint32_t *) &s_ntouched >= LIMIT) { s_overflow = 1; give_up = true; return false; }
        const uint32_t old = atomicCAS(&s_kf[slot].x, EMPTY_KEY, c);
        if (old == EMPTY_KEY) {
            const uint32_t idx = atomicAdd(&s_ntouched, 1u);
            if (idx < TOUCH_CAP) s_touched[idx] = (uint16_t) slot;
            if (idx >= LIMIT) s_overflow = 1;
            return true;
        }
        return old == c;
    };
    auto find_or_insert = [&](uint32_t c, uint32_t &seen_first) -> uint32_t {
        uint32_t slot = (c * 2654435761u) >> (32 - HT_BITS_);
        if constexpr (PROBE2) {
            // two slots per look (the big table's rows are bound by instruction issue, and this loop runs as often as its
            // unluckiest lane needs: half the trips for one more LDS read each)
            for (;;) {
                const uint32_t slot1 = (slot + 1) & (HT - 1);
                const uint2 k0 = s_kf[slot], k1 = s_kf[slot1];
                if (k0.x == c) { seen_first = k0.y; return slot; }
                bool give_up = false;
                if (k0.x == EMPTY_KEY) {
                    seen_first = 0;
                    if (claim(slot, c, give_up)) return slot;
                    if (give_up) return NO_SLOT;
                    // (someone else took it for another column: on to the next slot, whose key was read BEFORE that — look again)
                    slot = slot1;
                    continue;
                }
                if (k1.x == c) { seen_first = k1.y; return slot1; }
                if (k1.x == EMPTY_KEY) {
                    seen_first = 0;
                    if (claim(slot1, c, give_up)) return slot1;
                    if (give_up) return NO_SLOT;
                    slot = (slot1 + 1) & (HT - 1);
                    continue;
                }
                slot = (slot1 + 1) & (HT - 1);
            }
        } else {
        for (;;) {
            const uint2 kf = s_kf[slot];
            seen_first = kf.y;
            if (kf.x == c) return slot;
            if (kf.x == EMPTY_KEY) {
                bool give_up = false;
                if (claim(slot, c, give_up)) return slot;
                if (give_up) return NO_SLOT;
            }
            slot = (slot + 1) & (HT - 1);
        }
        }
    };
    auto add_to = [&](uint32_t slot, uint32_t seen_first, uint32_t cc, uint32_t mc, uint32_t finv) {
        if (track_first && seen_first < finv) atomicMax(&s_kf[slot].y, finv);
        const unsigned long long add = (unsigned long long) min(cc, mc) | ((unsigned long long) mc << 21) | ((unsigned long long) cc << 42);
        atomicAdd(&s_acc[slot], add);
    };
    // stage ranges [e0 + b0, e0 + b0 + nb) and return the number of lookups they hold
    auto stage = [&](uint32_t e0, uint32_t b0, uint32_t nb) -> uint32_t {
        uint32_t len[RPT], sum = 0;
        if (a.ranges8) {                                     // (uniform) packed ranges: half the bytes, the group named by its end
            uint2 rg8[RPT];
#pragma unroll
            for (uint32_t j = 0; j < RPT; j++) {             // the loads first, branch-free: they overlap
                const uint32_t i = tid * RPT + j;
                rg8[j] = a.ranges8[e0 + b0 + (i < nb ? i : nb - 1)];
            }
#pragma unroll
            for (uint32_t j = 0; j < RPT; j++) {
                const uint32_t i = tid * RPT + j;
                len[j] = 0;
                if (i < nb) {
                    s_gm[i] = rg8[j];                                    // as it is: the walk unpacks it (one LDS read per lookup instead of two)
                    len[j] = rg8[j].y & 0x3fffffu;
                }
                sum += len[j];
            }
        } else {
        uint4 rgs[RPT];
#pragma unroll
        for (uint32_t j = 0; j < RPT; j++) {                 // the loads first, branch-free: they overlap
            const uint32_t i = tid * RPT + j;
            rgs[j] = a.ranges[e0 + b0 + (i < nb ? i : nb - 1)];   // {first posting, postings, own count, group size}
        }
#pragma unroll
        for (uint32_t j = 0; j < RPT; j++) {
            const uint32_t i = tid * RPT + j;
            len[j] = 0;
            if (i < nb) {
                const uint4 rg = rgs[j];
                s_gm[i] = make_uint2(rg.x, rg.z); s_gsv[i] = rg.x + rg.y - rg.w; len[j] = rg.y;
            }
            sum += len[j];
        }
        }
        // exclusive prefix over the workgroup with ONE barrier: wave scans, wave totals through LDS, and every thread adds
        // up the (at most 16) totals of the waves before its own — the staging costs two barriers per batch, not five
        constexpr uint32_t NW = T / PDL_WAVE;
        const uint32_t inc = wave_inclusive_scan_u32(sum);
        if ((tid & (PDL_WAVE - 1)) == PDL_WAVE - 1) s_wave[tid / PDL_WAVE] = inc;
        pdl_sync();
        uint32_t total = 0, wave_off = 0;
#pragma unroll
        for (uint32_t w = 0; w < NW; w++) { const uint32_t t = s_wave[w]; wave_off += w < tid / PDL_WAVE ? t : 0u; total += t; }
        uint32_t ex = inc - sum + wave_off;
        // every wave walks a contiguous segment of the flat lookup space: segment w starts at lookup w * seg
        const uint32_t chunks = (total + PDL_WAVE - 1) / PDL_WAVE;
        const uint32_t seg = ((chunks + NW - 1) / NW) * PDL_WAVE;
#pragma unroll
        for (uint32_t j = 0; j < RPT; j++) {
            const uint32_t i = tid * RPT + j;
            s_cum[i] = i < nb ? ex : (i == nb ? total : 0xffffffffu);     // s_cum[nb] = total: > every flat index
            if (len[j]) {                                    // the range that holds a segment's first lookup registers itself
                uint32_t w_lo = 0;                                           // first w with w * seg >= ex
                if constexpr (NW <= 4) {                                     // (a few compares instead of an integer division per range)
#pragma unroll
                    for (uint32_t w = 0; w < NW; w++) w_lo += (uint32_t) (w * seg < ex);
                } else {
                    w_lo = seg ? (ex + seg - 1) / seg : 0;
                }
                for (uint32_t w = w_lo; w < NW && w * seg < ex + len[j]; w++) s_wstart[w] = make_uint2(i, ex);
            }
            ex += len[j];
        }
        if (tid == 0) s_cum[RB] = nb == RB ? total : 0xffffffffu;
        pdl_sync();
        return total;
    };
    // Walk the staged lookups; fn(posting, {group start, own count}).  Every wave owns a contiguous segment of
    // the flat lookup space and takes it 64 lookups (one per lane) at a time, four such chunks in flight.  The
    // range of each lane's lookup comes from ONE coalesced LDS read per chunk: lane l reads the start of range
    // rs+1+l (rs = range holding the chunk's first lookup, carried in scalar registers); the starts that fall
    // inside the chunk are turned into a 64-bit boundary mask with scalar ops, and a lane's range is rs +
    // popcount(boundaries at or below the lane), its offset the distance to the last such boundary.
    // a staged range as the lookups use it: gm.y = the row's own count of the k-mer, gsv = the value that names the group
    const bool packed = a.ranges8 != nullptr;
    auto unpack = [&](uint2 &gm, uint32_t &gsv, uint32_t r, bool live) {
        if (packed) {                                        // (uniform) {first posting, postings | min(own, 1023) << 22}: the group is named by its end
            gsv = gm.x + (gm.y & 0x3fffffu);
            gm.y >>= 22;
            if (__builtin_expect(gm.y == 1023u && live, 0)) gm.y = a.post[gm.x - 1].y & PDL_COUNT_MASK;       // (rare) the k-mer occurs >= 1023 times in this gene; (a dead lane holds no range)
        } else gsv = s_gsv[r];
    };
    auto walk = [&](uint32_t total, auto &&fn4) {
        constexpr uint32_t NW = T / PDL_WAVE;
        const uint32_t lane = tid & (PDL_WAVE - 1), wave = tid / PDL_WAVE;
        const uint32_t chunks = (total + PDL_WAVE - 1) / PDL_WAVE;
        const uint32_t cpw = (chunks + NW - 1) / NW;
        uint32_t ch = wave * cpw;
        const uint32_t ch_end = min(chunks, ch + cpw);
        if (ch >= ch_end) return;
        const uint2 ws = s_wstart[wave];
        uint32_t rs = __builtin_amdgcn_readfirstlane(ws.x);        // wave-uniform: range holding lookup ch * 64
        for (; ch < ch_end; ch += NCH) {
            if (*(volatile uint32_t *) &s_overflow) break;
            uint2 gm[NCH], po[NCH];
            uint32_t adr[NCH], gsv[NCH];
            bool live[NCH];
            const uint32_t nu = min(NCH, ch_end - ch);                    // chunks of this iteration (wave-uniform)
            const uint32_t f_lo = ch * PDL_WAVE, f_hi = f_lo + nu * PDL_WAVE;
            // ONE read of the next 64 range starts serves all four chunks when it reaches past them (always, unless
            // the ranges average under 4 postings): the four lane->range mappings then do not wait for each other.
            const uint32_t vw = s_cum[rs + 1 + lane];                    // starts of the following ranges (all > f_lo)
            if (__builtin_amdgcn_readlane(vw, PDL_WAVE - 1) >= f_hi) {
#pragma unroll
                for (uint32_t u = 0; u < NCH; u++) {
                    live[u] = false;
                    if (u < nu) {                                        // wave-uniform
                        const uint32_t lo = f_lo + u * PDL_WAVE, f = lo + lane;
                        const uint32_t cu = (uint32_t) __popcll(__ballot(vw <= lo));       // ranges that begin at or before the chunk
                        const bool inside = vw > lo && vw < lo + PDL_WAVE;
                        const int recv = __builtin_amdgcn_ds_permute((int) ((inside ? vw - lo : 0u) << 2), inside ? 1 : 0);
                        const unsigned long long m = __ballot(recv != 0);
                        // ranges that start at or before this lane's lookup: those up to the chunk's first one, the starts below the lane
                        // (mbcnt), its own; the offset inside the range from the range's start (one more LDS read, no scan of the mask)
                        const uint32_t r = rs + cu + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)) + (uint32_t) (recv != 0);
                        const uint32_t off = f - s_cum[r];
                        live[u] = f < total;
                        gm[u] = s_gm[r];
                        adr[u] = gm[u].x + off;
                        unpack(gm[u], gsv[u], r, live[u]);
#ifdef PDL_JOIN_CHECK
                        if (live[u] && !(s_cum[r] <= f && f < s_cum[r + 1] && off == f - s_cum[r])) atomicAdd(a.error_count, 1u);
#endif
                    }
                }
                const uint32_t ce = (uint32_t) __popcll(__ballot(vw <= f_hi));             // range holding the next iteration's first lookup
                rs += ce;
            } else {
#pragma unroll
            for (uint32_t u = 0; u < NCH; u++) {
                live[u] = false;
                if (ch + u < ch_end) {                   // wave-uniform: all 64 lanes are active in here
                    const uint32_t f0 = (ch + u) * PDL_WAVE, f = f0 + lane;
                    const uint32_t v = s_cum[rs + 1 + lane];            // starts of the following ranges (all > f0)
                    const bool inside = v < f0 + PDL_WAVE;              // a prefix of the lanes (starts ascend)
                    // scatter "a range starts here" to the lane at that position: LDS crossbar, no memory touched.
                    // Lanes without a start inside the chunk send 0 to lane 0, which is never a start position.
                    const int recv = __builtin_amdgcn_ds_permute((int) ((inside ? v - f0 : 0u) << 2), inside ? 1 : 0);
                    const unsigned long long m = __ballot(recv != 0);
                    const uint32_t w = (uint32_t) __popcll(__ballot(inside));
                    const uint32_t r = rs + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)) + (uint32_t) (recv != 0);
                    const uint32_t off = f - s_cum[r];
                    live[u] = f < total;
                    gm[u] = s_gm[r];
                    adr[u] = gm[u].x + off;
                    unpack(gm[u], gsv[u], r, live[u]);
#ifdef PDL_JOIN_CHECK
                    if (live[u] && !(s_cum[r] <= f && f < s_cum[r + 1] && off == f - s_cum[r])) atomicAdd(a.error_count, 1000u);
#endif
                    // keep the invariant "rs holds the first lookup of the next chunk": a range may start exactly there
                    const uint32_t nextb = w < PDL_WAVE ? __builtin_amdgcn_readlane(v, w) : s_cum[rs + 1 + PDL_WAVE];
                    rs += w + (uint32_t) (nextb == f0 + PDL_WAVE);
                }
            }
            }
            PH_WAIT(); PH_MARK(5);
#pragma unroll
            for (uint32_t u = 0; u < NCH; u++) po[u] = a.post[live[u] ? adr[u] : 0u];     // dead lanes (last chunk) read posting 0: no exec juggling
#pragma unroll
            for (uint32_t u = 0; u < NCH; u++) po[u].y &= PDL_COUNT_MASK;                 // (a group's head keeps its bit: MODE 0 gathers it)
            PH_WAIT(); PH_MARK(6);
#ifdef PDL_JOIN_CHECK
            if (*(volatile uint32_t *) &s_rowseq != my_seq) atomicAdd(a.error_count, 1000000u);
#endif
            fn4(po, gm, gsv, live);
#ifdef PDL_JOIN_CHECK
            if (*(volatile uint32_t *) &s_rowseq != my_seq) atomicAdd(a.error_count, 1000000u);
#endif
        }
    };

    for (;;) {
        pdl_sync();
        const uint32_t wi = s_next;
        const uint4 d = s_desc;
#ifdef PDL_JOIN_CHECK
        my_seq++;
        if (tid == 0) s_rowseq = my_seq;
#endif
        pdl_sync();
        PH_MARK(0);
        if (wi >= n_work) break;                         // uniform: every wave leaves here
        // the next row's ticket and descriptor are fetched now and parked in registers of lane 0 until the
        // end of this row, so the row after this one starts without a dependent global load
        uint32_t next_reg = 0;
        uint4 next_desc = make_uint4(0, 0, 0, 0);
        if (tid == 0) {
            next_reg = wi + 1;
            if (next_reg >= s_batch_end) {               // batch used up: take the next one
                next_reg = atomicAdd(a.work_cursor, a.work_batch);
                s_batch_end = next_reg + a.work_batch;
            }
            if (next_reg < n_work) next_desc = a.desc[next_reg];
        }
        const uint32_t p = d.x, r = d.y, e0 = d.z, nr = d.w;
        if (nr == 0) {                                   // gene shares no k-mer group: no candidates
            if (tid == 0) { a.row_base[p] = 0; a.row_cnt[p] = 0; s_next = next_reg; s_desc = next_desc; }
            continue;
        }
        const uint4 row_info = a.gene_info[r];
        const uint32_t my_kcnt = row_info.x;
        // ---- lookups (library.cpp:461-479) -----------------------------------------------------------
        if constexpr (!FILTER) {
            for (uint32_t b0 = 0; b0 < nr; b0 += RB) {
                const uint32_t total = stage(e0, b0, min(RB, nr - b0));
                walk(total, [&](const uint2 (&po)[NCH], const uint2 (&gm)[NCH], const uint32_t (&gsv)[NCH], const bool (&live)[NCH]) {
#pragma unroll
                    for (uint32_t u = 0; u < NCH; u++) {
                        if (!live[u]) continue;
                        uint32_t seen;
                        const uint32_t slot = find_or_insert(po[u].x, seen);
                        if (slot != NO_SLOT) add_to(slot, seen, po[u].y, gm[u].y, 0xffffffffu - gsv[u]);
                    }
                });
                pdl_sync();
            }
        } else {
            // single-sighting columns may be dropped only if nobody involved has <= 2k k-mers
            const bool filter_on = my_kcnt > 2 * a.k && a.min_kseq > 2 * a.k;
            for (uint32_t i = tid; i < Cfg::BM_WORDS / 4; i += T) reinterpret_cast<uint4 *>(s_bm)[i] = make_uint4(0, 0, 0, 0);
            constexpr uint32_t NWV = T / PDL_WAVE;
            const uint32_t wcap = a.defer_cap / NWV;               // every wave files its own part of the list: the count stays in a scalar register
            // entry of the list: 8 bytes {column | 10-bit tag << 22, group} when gene ids fit 22 bits, else 16 {column, group, row, launch}
            const bool wide_list = a.defer_wide != 0;
            const size_t wlist0 = (size_t) blockIdx.x * a.defer_cap + (size_t) (tid / PDL_WAVE) * wcap;
            uint4 *wdefer16 = reinterpret_cast<uint4 *>(a.defer) + wlist0;
            uint2 *wdefer8 = reinterpret_cast<uint2 *>(a.defer) + wlist0;
            const uint32_t tag10 = ((p + 389u * a.defer_serial) & 1023u) << 22;
            uint32_t nd_w = 0;
            const uint32_t lane = tid & (PDL_WAVE - 1);
            const unsigned long long lt_mask = (1ull << lane) - 1ull;
            // ONE walk.  A light lookup (both counts 1) whose column's bit is still clear is the column's first sighting: it
            // sets the bit and is put aside — {column, group} appended to its wave's part of this workgroup's list in HBM
            // (coalesced; the count is a scalar register; the list is rewritten row after row, it lives in L2).  Every other lookup
            // (a heavy one, or the bit is already set: a second sighting, or another column's bit under a hash collision)
            // gets a slot and is added at once.  When the walk is over the kept columns are known, and the lookups put
            // aside are looked up in the table: those whose column has a slot add their (1, 1, 1), the others are the
            // single sightings that cannot be emitted.  Every lookup is counted exactly once either way.
            for (uint32_t b0 = 0; b0 < nr; b0 += RB) {
                const uint32_t total = stage(e0, b0, min(RB, nr - b0));     // (its barriers also cover the bitmap clear)
                PH_MARK(1);
                walk(total, [&](const uint2 (&po)[NCH], const uint2 (&gm)[NCH], const uint32_t (&gsv)[NCH], const bool (&live)[NCH]) {
                    bool ins[NCH], later[NCH];
                    uint32_t old[NCH], bit[NCH];
#pragma unroll
                    for (uint32_t u = 0; u < NCH; u++) {       // four bitmap atomics in flight
                        ins[u] = live[u] && (!filter_on || max(po[u].y, gm[u].y) >= 2);
                        const uint32_t h = (po[u].x * 0x9E3779B1u) >> (32 - Cfg::BM_BITS_LOG2);
                        bit[u] = 1u << (h & 31);
                        old[u] = (live[u] && !ins[u]) ? atomicOr(&s_bm[h >> 5], bit[u]) : 0u;
                    }
                    PH_WAIT(); PH_MARK(7);
                    unsigned long long m[NCH];
                    uint32_t n_later = 0;
#pragma unroll
                    for (uint32_t u = 0; u < NCH; u++) {
                        later[u] = live[u] && !ins[u] && !(old[u] & bit[u]);
                        m[u] = __ballot(later[u]);
                        n_later += (uint32_t) __popcll(m[u]);
                    }
                    uint32_t at = nd_w;
                    nd_w += n_later;
                    if (nd_w > wcap) s_overflow = 1;             // (wave-uniform) no room for this iteration's first sightings: next tier
#pragma unroll
                    for (uint32_t u = 0; u < NCH; u++) {
                        if (later[u]) {
                            const uint32_t i = at + (uint32_t) __popcll(m[u] & lt_mask);
                            if (i < wcap) {
                                if (wide_list) wdefer16[i] = make_uint4(po[u].x, 0xffffffffu - gsv[u], p, a.defer_serial);
                                else wdefer8[i] = make_uint2(po[u].x | tag10, 0xffffffffu - gsv[u]);
                            }
                        } else if (live[u]) {
                            uint32_t seen;
                            const uint32_t slot = find_or_insert(po[u].x, seen);
                            if (slot != NO_SLOT) add_to(slot, seen, po[u].y, gm[u].y, 0xffffffffu - gsv[u]);
                        }
                        at += (uint32_t) __popcll(m[u]);
                    }
#ifdef PDL_JOIN_PHASES
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); PH_MARK(8);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); PH_MARK(9);
#endif
                });
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the wave's stores to its list have been acknowledged by L2 before it reads them back
                pdl_sync();
                PH_MARK(2);
            }
            if (!s_overflow) {
                // The lookups put aside: add the ones whose column was kept.  Every wave goes through the part of the list
                // it wrote itself — nothing here depends on seeing another wave's global stores; the barrier above is for
                // the table, which all waves fill.  The list is rewritten row after row, so what a load must not return is
                // the PREVIOUS content of an entry.  Twice that has happened (first with cross-wave reads behind a fence and
                // a barrier, then — rarely, and only after an unrelated edit changed the kernel's timing — with a wave
                // reading back its own `sc1` stores, which leave L2 for the fabric while an `sc1` load that misses L2 can
                // reach memory before them).  So: plain stores (write-through L1, the line STAYS in this XCD's L2), `sc1` loads
                // (never served by L1, so L2 it is) — a wave's own stores, acknowledged by L2, then its own loads from L2 —
                // and every entry carries a tag of the row (and launch) it was written for: one that does not show it is
                // loaded again, and counted (pdl_timings.aside_reloads — the canary: 0 in every run so far).  16-byte entries
                // carry row and launch in full; the 8-byte ones (gene ids below 2^22: every BASELINE set) have room for
                // ten bits, which tell a previous row's entry 1023 times in 1024 — enough for the canary to go off long
                // before a stale entry could pass, and configs[4]'s join pays 36 % for the other eight bytes.  A load that
                // never shows the tag gives up and counts an error (the host fails the pass).
                for (uint32_t i0 = 0; i0 < nd_w; i0 += 4 * PDL_WAVE) {
                    uint32_t col[4], grp[4], slot[4];
                    uint2 kf[4];
                    bool have[4];
                    uint32_t at[4];
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) {
                        const uint32_t i = i0 + u * PDL_WAVE + lane;
                        have[u] = i < nd_w;
                        at[u] = have[u] ? i : 0u;
                    }
                    if (wide_list) {                             // (uniform)
                        u32x4 e[4];
                        const uint4 *src[4] = {&wdefer16[at[0]], &wdefer16[at[1]], &wdefer16[at[2]], &wdefer16[at[3]]};
                        ld16_sc1_x4(src, e);                     // four loads in flight, one wait
#pragma unroll
                        for (uint32_t u = 0; u < 4; u++) {
                            uint32_t tries = 0;
                            while (have[u] && (e[u].z != p || e[u].w != a.defer_serial)) {   // not (yet) what this wave stored there for this row
                                if (tries == 0) atomicAdd(a.reload_count, 1u);
                                if (++tries > 4096u) { atomicAdd(a.error_count, 1u); have[u] = false; break; }
                                e[u] = ld16_sc1(src[u]);
                            }
                            col[u] = e[u].x; grp[u] = e[u].y;
                        }
                    } else {
                        unsigned long long e[4];
#pragma unroll
                        for (uint32_t u = 0; u < 4; u++) e[u] = ld_agent(reinterpret_cast<const unsigned long long *>(&wdefer8[at[u]]));
#pragma unroll
                        for (uint32_t u = 0; u < 4; u++) {
                            uint32_t tries = 0;
                            while (have[u] && ((uint32_t) e[u] & 0xffc00000u) != tag10) {
                                if (tries == 0) atomicAdd(a.reload_count, 1u);
                                if (++tries > 4096u) { atomicAdd(a.error_count, 1u); have[u] = false; break; }
                                e[u] = ld_agent(reinterpret_cast<const unsigned long long *>(&wdefer8[at[u]]));
                            }
                            col[u] = (uint32_t) e[u] & 0x3fffffu; grp[u] = (uint32_t) (e[u] >> 32);
                        }
                    }
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) {       // four first probes in flight
                        slot[u] = (col[u] * 2654435761u) >> (32 - HT_BITS_);
                        kf[u] = s_kf[slot[u]];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < 4; u++) {
                        if (!have[u]) continue;
                        for (;;) {
                            if (kf[u].x == col[u]) { add_to(slot[u], kf[u].y, 1u, 1u, grp[u]); break; }
                            if (kf[u].x == EMPTY_KEY) break;         // column was seen once only
                            slot[u] = (slot[u] + 1) & (HT - 1);
                            kf[u] = s_kf[slot[u]];
                        }
                    }
                }
            }
            pdl_sync();
        }
        PH_MARK(3);
        const uint32_t ntouched = min(s_ntouched, TOUCH_CAP);
        if (s_overflow) {
            // too many keys for this table: hand the row to the next tier, wipe the table
            if (tid == 0) { const uint32_t oi = atomicAdd(a.overflow_count, 1u); a.overflow_rows[oi] = p; if (a.overflow_desc) a.overflow_desc[oi] = d; }
            pdl_sync();
            for (uint32_t i = tid; i < HT; i += T) { s_kf[i] = make_uint2(EMPTY_KEY, 0u); s_acc[i] = 0; }
            if (tid == 0) { s_ntouched = 0; s_nemit = 0; s_overflow = 0; s_next = next_reg; s_desc = next_desc; }
            continue;
        }
        // ---- finalize + emit (library.cpp:485-517) ------------------------------------------------
        // The staging chunk of this workgroup must have room for every touched candidate, so cells can be
        // written where they are decided; a fresh chunk is taken otherwise (its tail stays unused).
        if (tid == 0) {
            unsigned long long nx = s_chunk_next;
            if (nx + ntouched > s_chunk_end) {
                nx = atomicAdd(a.cell_cursor, (unsigned long long) CELL_CHUNK);
                s_chunk_end = nx + CELL_CHUNK;
                s_chunk_next = nx;
            }
            s_base = nx;
        }
        const uint32_t pc_min = min_numerator(threshold, (float) (int) my_kcnt);
        const uint32_t my_genome = row_info.y;
        float *ms_row = a.MS + (size_t) p * a.G;
        float *cm_row = a.CM + (size_t) row_info.w * a.N;
        pdl_sync();
        const unsigned long long base = s_base;
        const bool fits = base + ntouched <= a.st_cap;
        for (uint32_t t = tid; t < ntouched; t += T) {
            const uint32_t slot = s_touched[t];
            const uint2 kf = s_kf[slot];
            const uint32_t c = kf.x;
            const unsigned long long acc = s_acc[slot];
            s_kf[slot] = make_uint2(EMPTY_KEY, 0u); s_acc[slot] = 0;        // slot consumed
            if (c >= a.N) { atomicAdd(a.error_count, 1u); continue; }       // a listed slot must hold a column id
            if (c == r) continue;                         // identity cell is zeroed (library.cpp:485-487)
            // score_valid needs perc >= thr or tr_perc >= thr (library.cpp:497-500).  Both quotients are monotone
            // in their numerators, and tr_perc = tc / K_c <= tc / min_kseq (IEEE division is monotone in the
            // divisor), so two integer compares against thresholds derived with the same float expressions
            // drop a candidate without a division or a fetch of K_c.
            if ((uint32_t) ((acc >> 21) & FIELD_MASK) < pc_min && (uint32_t) (acc >> 42) < tc_min) continue;
            float perc, tr;
            const uint4 ci = a.gene_info[c];
            const float score = finalize_cell(acc, my_kcnt, ci.x, threshold, perc, tr);
            if (score > 0.0f) {
                const uint32_t i = atomicAdd(&s_nemit, 1u);
                if (fits) {
                    const unsigned long long o = base + i;
                    a.st_score[o] = score; a.st_perc[o] = perc; a.st_tr[o] = tr;
                    a.st_col[o] = c; a.st_first[o] = 0xffffffffu - kf.y;
                    // scores are positive floats: their bit patterns order like the values
                    const uint32_t gc = ci.y;
                    atomicMax(reinterpret_cast<uint32_t *>(ms_row + gc), __float_as_uint(score));
                    atomicMax(reinterpret_cast<uint32_t *>(cm_row + c), __float_as_uint(score));
                    if (a.mirror) {
                        // the same sums seen from gene c: cell (c, r) with perc and tr_perc swapped (both quotients
                        // use the same integers the row program of c would have summed); K-order places it in c's row.
                        // Multi-GPU: when c is another GPU's row the staged cell travels there (k_outbox_*).
                        const uint32_t pc = ci.z;
                        if (pc != 0xffffffffu) {
                            atomicAdd(&a.mirror_cnt[pc], 1u);
                            atomicMax(reinterpret_cast<uint32_t *>(a.MS + (size_t) pc * a.G + my_genome), __float_as_uint(score));
                            atomicMax(reinterpret_cast<uint32_t *>(a.CM + (size_t) ci.w * a.N + r), __float_as_uint(score));
                        }
                    }
                }
            }
        }
        pdl_sync();
        PH_MARK(4);
        if (tid == 0) {
            const uint32_t nemit = s_nemit;
            a.row_base[p] = fits ? (uint32_t) base : 0u;
            a.row_cnt[p] = fits ? nemit : 0u;       // staging ran out: the row holds nothing (the host repeats the pass with the
                                                    // size asked for); everything queued behind the join stays inside its buffers
            s_chunk_next = base + nemit;
            s_ntouched = 0; s_nemit = 0; s_next = next_reg; s_desc = next_desc;
        }
    }
#ifdef PDL_JOIN_PHASES
    if (tid == 0 && a.phase) { for (int i = 0; i < 10; i++) atomicAdd(&a.phase[i], ph[i]); }
#endif
#undef PH_MARK
#undef PH_WAIT
}

// ------------------------------------------------------------------------------------------------
// K-join (HBM tables): direct-addressed by column id, private to the workgroup (one CU, one XCD, one L2).  Every update of
// the tables is an L2-level atomic or a PLAIN store (write-through L1, the line stays in that L2), every read an `sc1`
// load (never served by L1), and a storing wave waits for its stores (vmcnt) before the barrier that hands them over: the
// workgroup sees its own updates in L2.  No `sc1` STORES: they send the line out of L2 to the fabric, and a load or an
// atomic that then misses L2 can reach memory before them (seen in the LDS tier's put-aside list).  Tables are all-zero
// between rows.
// ------------------------------------------------------------------------------------------------

// WIDE = true keeps the three sums in separate 32-bit counters (the reference's int arrays, library.cpp:421-423) instead of
// the packed 21-bit fields: the only path for datasets with a gene of >= 2^20 k-mers, where every row is sent here.
template <bool WIDE>
__global__ __launch_bounds__(HBM_THREADS) void k_join_hbm(JoinArgs a) {
    constexpr int JOIN_THREADS = HBM_THREADS;
    __shared__ uint32_t s_ntouched, s_nemit, s_work, s_batch_end;
    __shared__ unsigned long long s_base;
    const uint32_t tid = threadIdx.x;
    unsigned long long *t_acc = a.hbm_acc + (size_t) blockIdx.x * (WIDE ? 2 : 1) * a.N;      // WIDE: u32 [3][N] in the same bytes (+ N spare)
    uint32_t *t_w = reinterpret_cast<uint32_t *>(t_acc);
    uint32_t *t_first = a.hbm_u32 + (size_t) blockIdx.x * 3 * a.N;
    auto read_cell = [&](uint32_t c, uint32_t my_kcnt, float threshold, float &perc, float &tr) -> float {
        if constexpr (WIDE)
            return finalize_counts((int) ld_agent(&t_w[c]), (int) ld_agent(&t_w[a.N + c]), (int) ld_agent(&t_w[2 * (size_t) a.N + c]),
                                   my_kcnt, a.kseq_len[c], threshold, perc, tr);
        else
            return finalize_cell(ld_agent(&t_acc[c]), my_kcnt, a.kseq_len[c], threshold, perc, tr);
    };
    uint32_t *t_touched = t_first + a.N;
    uint32_t *t_emit = t_touched + a.N;
    if (tid == 0) { s_ntouched = 0; s_nemit = 0; s_work = 0xffffffffu; s_batch_end = 0; }
    const float threshold = 1.0f / (2.0f * (float) a.k);
    const uint32_t n_work = a.n_work_ptr ? *a.n_work_ptr : a.n_work;
    pdl_sync();
    for (;;) {
        if (tid == 0) {
            uint32_t nx = s_work + 1;
            if (nx >= s_batch_end) { nx = atomicAdd(a.work_cursor, a.work_batch); s_batch_end = nx + a.work_batch; }
            s_work = nx;
        }
        pdl_sync();
        const uint32_t wi = s_work;
        if (wi >= n_work) break;
        const uint32_t p = a.work[wi];
        const uint32_t r = a.task_rows[p];
        const uint32_t e0 = a.seq_off[r], e1 = a.seq_off[r + 1];
        // one wave per range; the whole workgroup strides over the long ones implicitly via wave count
        const uint32_t wave = tid / PDL_WAVE, lane = tid % PDL_WAVE, nwaves = JOIN_THREADS / PDL_WAVE;
        for (uint32_t e = e0 + wave; e < e1; e += nwaves) {
            uint4 rg;                                         // {first posting, postings, own count, group size}
            uint32_t group_key;                               // names the group in rank order: its start, or (packed ranges) its end
            if (a.ranges8) {
                const uint2 r8 = a.ranges8[e];
                uint32_t own = r8.y >> 22;
                if (own == 1023u) own = a.post[r8.x - 1].y & PDL_COUNT_MASK;
                rg = make_uint4(r8.x, r8.y & 0x3fffffu, own, 0u);
                group_key = rg.x + rg.y;
            } else {
                rg = a.ranges[e];
                group_key = rg.x + rg.y - rg.w;
            }
            const uint32_t finv = 0xffffffffu - group_key;
            for (uint32_t q = lane; q < rg.y; q += PDL_WAVE) {
                uint2 po = a.post[rg.x + q];
                po.y &= PDL_COUNT_MASK;
                const uint32_t c = po.x;
                if (ld_agent(&t_first[c]) < finv) {
                    const uint32_t old = atomicMax(&t_first[c], finv);
                    if (old == 0) {                                                // first toucher lists the column
                        const uint32_t idx = atomicAdd(&s_ntouched, 1u);
                        if (idx < a.N) t_touched[idx] = c; else atomicAdd(a.error_count, 1u);
                    }
                }
                if constexpr (WIDE) {
                    atomicAdd(&t_w[c], min(po.y, rg.z));
                    atomicAdd(&t_w[a.N + c], rg.z);
                    atomicAdd(&t_w[2 * (size_t) a.N + c], po.y);
                } else {
                    const unsigned long long add = (unsigned long long) min(po.y, rg.z) | ((unsigned long long) rg.z << 21) | ((unsigned long long) po.y << 42);
                    atomicAdd(&t_acc[c], add);
                }
            }
        }
        __threadfence();      // the touched list was written with plain stores by other waves of this workgroup
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        pdl_sync();
        const uint32_t ntouched = min(s_ntouched, a.N);
        const uint32_t my_kcnt = a.kseq_len[r];
        for (uint32_t t = tid; t < ntouched; t += JOIN_THREADS) {
            const uint32_t c = ld_agent(&t_touched[t]);
            if (c == r || c >= a.N) continue;
            float perc, tr;
            const float score = read_cell(c, my_kcnt, threshold, perc, tr);
            if (score > 0.0f) {
                const uint32_t idx = atomicAdd(&s_nemit, 1u);
                if (idx < a.N) t_emit[idx] = c;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (a barrier does not wait for stores)
        pdl_sync();
        const uint32_t nemit = min(s_nemit, a.N);
        if (tid == 0) {
            const unsigned long long base = atomicAdd(a.cell_cursor, (unsigned long long) nemit);
            s_base = base;
            const bool fits = base + nemit <= a.st_cap;     // else: nothing is staged, the host repeats the pass
            a.row_base[p] = fits ? (uint32_t) base : 0u;
            a.row_cnt[p] = fits ? nemit : 0u;
        }
        pdl_sync();
        const unsigned long long base = s_base;
        if (base + nemit <= a.st_cap) {
            float *ms_row = a.MS + (size_t) p * a.G;
            float *cm_row = a.CM + (size_t) a.task_lg[p] * a.N;
            for (uint32_t i = tid; i < nemit; i += JOIN_THREADS) {
                const uint32_t c = ld_agent(&t_emit[i]);
                float perc, tr;
                const float score = read_cell(c, my_kcnt, threshold, perc, tr);
                const unsigned long long o = base + i;
                a.st_score[o] = score; a.st_perc[o] = perc; a.st_tr[o] = tr;
                a.st_col[o] = c; a.st_first[o] = 0xffffffffu - ld_agent(&t_first[c]);
                const uint32_t gc = a.genome_of[c];
                atomicMax(reinterpret_cast<uint32_t *>(ms_row + gc), __float_as_uint(score));
                atomicMax(reinterpret_cast<uint32_t *>(cm_row + c), __float_as_uint(score));
                if (a.mirror) {      // cell (c, r), see k_join_lds
                    const uint32_t pc = a.taskpos_of[c];
                    if (pc != 0xffffffffu) {
                        atomicAdd(&a.mirror_cnt[pc], 1u);
                        atomicMax(reinterpret_cast<uint32_t *>(a.MS + (size_t) pc * a.G + a.genome_of[r]), __float_as_uint(score));
                        atomicMax(reinterpret_cast<uint32_t *>(a.CM + (size_t) a.local_genome[gc] * a.N + r), __float_as_uint(score));
                    }
                }
            }
        }
        pdl_sync();
        for (uint32_t t = tid; t < ntouched; t += JOIN_THREADS) {
            const uint32_t c = ld_agent(&t_touched[t]);
            if (c < a.N) {
                if constexpr (WIDE) { t_w[c] = 0u; t_w[a.N + c] = 0u; t_w[2 * (size_t) a.N + c] = 0u; }
                else t_acc[c] = 0ull;
                t_first[c] = 0u;
            }
        }
        if (tid == 0) { s_ntouched = 0; s_nemit = 0; }
        __threadfence();      // the zeroing stores must have landed (in L2) before the next row's atomics
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        pdl_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// K-order: cells of task position p move from the staging area (arrival order) to
// fin_off[p] + rank, rank = position in the reference's emission order.  The reference visits columns
// chunk by chunk of 2048 ids ("<= max_allowed_sequence": chunk 0 is ids 0..2048, library.cpp:456-464),
// inside a chunk range by range, inside a range by ascending gene; a cell is emitted where its column
// is first touched.  Key = (chunk(col), first group start, col); canonical mode: key = col.
// Rank by counting over LDS tiles of the row's keys.
// ------------------------------------------------------------------------------------------------
constexpr int ORDER_THREADS = 256;
constexpr int ORDER_TILE = 2048;
constexpr uint32_t ORDER_CPL = 4;                              // cells per lane in the wave-per-row kernel
constexpr uint32_t ORDER_WAVE_CELLS = ORDER_CPL * PDL_WAVE;    // rows up to this many cells are ranked inside one wave

constexpr uint32_t ORDER_SUB_W = 16;                           // option "order_subwave" 1: lanes per short row
static uint32_t order_sub_w(const pdl_ctx *c) { return c->opt_order_subwave == 1 ? ORDER_SUB_W : (uint32_t) c->opt_order_subwave; }      // 0 | 16 | 32

struct MCell { uint32_t col, first; float score, perc, tr; uint32_t pad; };       // a mirrored cell as its row reads it (24 bytes)
struct OrderArgs {
    const uint32_t *row_base, *row_cnt, *fin_off, *task_rows;
    const float *st_score, *st_perc, *st_tr;
    const uint32_t *st_col, *st_first;
    // mirror mode: row p also owns mirror_cnt[p] cells that other rows staged; mcell holds them from mirror_off[p] on
    const uint32_t *mirror_cnt, *mirror_off;
    const MCell *mcell;
    float *c_score, *c_perc, *c_tr;
    int32_t *c_row, *c_col;
    uint32_t n_rows;
    uint32_t canonical;
    uint32_t pack_ok;                   // fewer than 2^22 genes: (chunk, first group, column) fits one 64-bit key
    uint32_t *wide_rows;                // set by k_order_rows_wave when it leaves a row to k_order_rows
};

__device__ __forceinline__ unsigned long long order_key_hi(uint32_t col, uint32_t first, uint32_t canonical) {
    if (canonical) return 0ull;
    const uint32_t chunk = col == 0 ? 0u : (col - 1) >> 11;
    return ((unsigned long long) chunk << 32) | first;
}

// the whole key in 64 bits when the gene ids allow it: chunk (11 bits) | first group (32) | column inside the chunk (12, 0..2048)
__device__ __forceinline__ unsigned long long order_key_packed(uint32_t col, uint32_t first, uint32_t canonical) {
    if (canonical) return col;
    const uint32_t chunk = col == 0 ? 0u : (col - 1) >> 11;
    return ((unsigned long long) chunk << 44) | ((unsigned long long) first << 12) | (col - (chunk << 11));
}

// cell i of row p: its own staged cells first (the staging arrays, at row_base[p] + i), then the mirrored ones — the
// staged cells of other rows as this row reads them (row/column and perc/tr_perc swapped), which k_mirror_cells has
// COPIED into this row's stretch of `mcell`: K-order reads every cell of a row from consecutive addresses (it used to
// follow a reference to the other row's staging slot: five dependent 4-byte gathers per mirrored cell).
struct OrderCell { uint32_t slot; bool mirrored; };
__device__ __forceinline__ OrderCell order_cell(const OrderArgs &a, uint32_t p, uint32_t own, uint32_t i) {
    if (i < own) return OrderCell{a.row_base[p] + i, false};
    return OrderCell{a.mirror_off[p] + (i - own), true};
}
__device__ __forceinline__ uint2 cell_key(const OrderArgs &a, const OrderCell &oc) {          // {column, first group}
    if (oc.mirrored) { const MCell &m = a.mcell[oc.slot]; return make_uint2(m.col, m.first); }
    return make_uint2(a.st_col[oc.slot], a.st_first[oc.slot]);
}
__device__ __forceinline__ void cell_values(const OrderArgs &a, const OrderCell &oc, float &score, float &perc, float &tr) {
    if (oc.mirrored) { const MCell &m = a.mcell[oc.slot]; score = m.score; perc = m.perc; tr = m.tr; }
    else { score = a.st_score[oc.slot]; perc = a.st_perc[oc.slot]; tr = a.st_tr[oc.slot]; }
}

// a row of more than ORDER_WAVE_CELLS cells (`own` of them its own), by the whole workgroup
__device__ __forceinline__ void order_wide_row(const OrderArgs &a, uint32_t p, uint32_t own, uint32_t cnt) {
    __shared__ unsigned long long s_hi[ORDER_TILE];
    __shared__ uint32_t s_col[ORDER_TILE];
    pdl_sync();                             // the LDS tiles of the previous row are done with
    const uint32_t out0 = a.fin_off[p];
    const uint32_t row = a.task_rows[p];
    if (a.pack_ok && cnt <= 512) {
        // rows of 257 to 512 cells (every row of a 512-genome set) when gene ids fit 22 bits: the 55-bit packed key and the
        // cell's 9-bit index are ONE 64-bit word — the bitonic network swaps one LDS array instead of three, compares once
        // (the index makes every key unique), and the column comes back out of the key
        for (uint32_t j = threadIdx.x; j < 512; j += ORDER_THREADS) {
            unsigned long long key = ~0ull;                      // padding sorts last
            if (j < cnt) {
                const uint2 kj = cell_key(a, order_cell(a, p, own, j));
                key = (order_key_packed(kj.x, kj.y, a.canonical) << 9) | j;
            }
            s_hi[j] = key;
        }
        pdl_sync();
        uint32_t prev_j = 2 * PDL_WAVE;
        bool first = true;
        for (uint32_t k = 2; k <= 512; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                if (!first) {
                    if (j > PDL_WAVE || prev_j > PDL_WAVE) pdl_sync();             // (see the general network below)
                    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                first = false; prev_j = j;
                const uint32_t t = threadIdx.x;                   // 256 pairs, one per thread
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi_i = lo | j;
                const unsigned long long ka = s_hi[lo], kb = s_hi[hi_i];
                if ((ka > kb) == ((lo & k) == 0)) { s_hi[lo] = kb; s_hi[hi_i] = ka; }
            }
        }
        pdl_sync();
        for (uint32_t q = threadIdx.x; q < cnt; q += ORDER_THREADS) {
            const unsigned long long key = s_hi[q];
            const unsigned long long pk = key >> 9;
            const uint32_t col = a.canonical ? (uint32_t) pk : ((uint32_t) (pk >> 44) << 11) + (uint32_t) (pk & 0xfffu);
            const OrderCell me = order_cell(a, p, own, (uint32_t) (key & 511u));
            const uint32_t o = out0 + q;
            float v_score, v_perc, v_tr;
            cell_values(a, me, v_score, v_perc, v_tr);
            a.c_score[o] = v_score; a.c_perc[o] = v_perc; a.c_tr[o] = v_tr;
            a.c_row[o] = (int32_t) row;
            a.c_col[o] = (int32_t) col;
        }
        return;
    }
    if (cnt <= ORDER_TILE) {
        // bitonic sort of the row's keys in LDS (keys are unique: the column is part of them); position q of the sorted
        // order then fetches its cell and writes output slot q — coalesced writes, O(n log^2 n) compares
        __shared__ uint16_t s_idx[ORDER_TILE];
        uint32_t n2 = 512;
        while (n2 < cnt) n2 <<= 1;
        for (uint32_t j = threadIdx.x; j < n2; j += ORDER_THREADS) {
            if (j < cnt) {
                const OrderCell oc = order_cell(a, p, own, j);
                const uint2 kj = cell_key(a, oc);
                const uint32_t cj = kj.x;
                s_col[j] = cj;
                s_hi[j] = order_key_hi(cj, kj.y, a.canonical);
            } else {
                s_col[j] = 0xffffffffu; s_hi[j] = ~0ull;         // padding sorts last
            }
            s_idx[j] = (uint16_t) j;
        }
        pdl_sync();
        // Pair t of a stage is handled by thread t mod 256, and for j <= 64 both of its elements lie in the 128-element block
        // of pair-group t / 64: such a stage moves data inside the block one wave owns, so two of them in a row need no
        // workgroup barrier between them (a wave's LDS operations execute in order) — 7 barriers for 512 keys instead of 46.
        uint32_t prev_j = 2 * PDL_WAVE;                          // (the load above was done by arbitrary threads)
        bool first = true;
        for (uint32_t k = 2; k <= n2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                if (!first) {
                    if (j > PDL_WAVE || prev_j > PDL_WAVE) pdl_sync();
                    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own exchanges of the stage before
                }
                first = false; prev_j = j;
                for (uint32_t t = threadIdx.x; t < n2 / 2; t += ORDER_THREADS) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi_i = lo | j;
                    const bool up = (lo & k) == 0;               // ascending block
                    const unsigned long long ha = s_hi[lo], hb = s_hi[hi_i];
                    const uint32_t ca = s_col[lo], cb = s_col[hi_i];
                    const bool a_gt_b = ha > hb || (ha == hb && ca > cb);
                    if (a_gt_b == up) {
                        s_hi[lo] = hb; s_hi[hi_i] = ha; s_col[lo] = cb; s_col[hi_i] = ca;
                        const uint16_t ia = s_idx[lo]; s_idx[lo] = s_idx[hi_i]; s_idx[hi_i] = ia;
                    }
                }
            }
        }
        pdl_sync();
        for (uint32_t q = threadIdx.x; q < cnt; q += ORDER_THREADS) {
            const OrderCell me = order_cell(a, p, own, s_idx[q]);
            const uint32_t o = out0 + q;
            float v_score, v_perc, v_tr;
            cell_values(a, me, v_score, v_perc, v_tr);
            a.c_score[o] = v_score; a.c_perc[o] = v_perc; a.c_tr[o] = v_tr;
            a.c_row[o] = (int32_t) row;
            a.c_col[o] = (int32_t) s_col[q];
        }
        return;
    }
    for (uint32_t i0 = 0; i0 < cnt; i0 += ORDER_THREADS) {
        const uint32_t i = i0 + threadIdx.x;
        const bool live = i < cnt;
        uint32_t col = 0;
        unsigned long long hi = 0;
        OrderCell me{0, false};
        if (live) {
            me = order_cell(a, p, own, i);
            const uint2 km = cell_key(a, me);
            col = km.x;
            hi = order_key_hi(col, km.y, a.canonical);
        }
        uint32_t rank = 0;
        for (uint32_t j0 = 0; j0 < cnt; j0 += ORDER_TILE) {
            const uint32_t tn = min((uint32_t) ORDER_TILE, cnt - j0);
            pdl_sync();
            for (uint32_t j = threadIdx.x; j < tn; j += ORDER_THREADS) {
                const OrderCell oc = order_cell(a, p, own, j0 + j);
                const uint2 kj = cell_key(a, oc);
                const uint32_t cj = kj.x;
                s_col[j] = cj;
                s_hi[j] = order_key_hi(cj, kj.y, a.canonical);
            }
            pdl_sync();
            if (live) {
                for (uint32_t j = 0; j < tn; j++) {          // broadcast reads; the column only breaks (rare) ties
                    const unsigned long long hj = s_hi[j];
                    if (hj < hi) rank++;
                    else if (hj == hi) rank += s_col[j] < col;
                }
            }
        }
        if (live) {
            const uint32_t o = out0 + rank;
            float v_score, v_perc, v_tr;
            cell_values(a, me, v_score, v_perc, v_tr);
            a.c_score[o] = v_score; a.c_perc[o] = v_perc; a.c_tr[o] = v_tr;
            a.c_row[o] = (int32_t) row;
            a.c_col[o] = (int32_t) col;
        }
    }
}
__global__ __launch_bounds__(ORDER_THREADS) void k_order_rows(OrderArgs a) {
    if (*a.wide_rows == 0) return;               // no row is wider than the wave kernel's limit (the usual case)
    for (uint32_t p = blockIdx.x; p < a.n_rows; p += gridDim.x) {       // persistent workgroups: rows dealt round-robin
        const uint32_t own = a.row_cnt[p];
        const uint32_t cnt = own + (a.mirror_cnt ? a.mirror_cnt[p] : 0u);
        if (cnt > ORDER_WAVE_CELLS) order_wide_row(a, p, own, cnt);       // (the others: k_order_rows_wave's rows; uniform)
    }
}
// The same without the counter, for workgroups that share a launch with the short rows' ones: workgroup `block` of `n_blocks` has
// the rows k_order_rows would deal it (block, block + n_blocks, ...) and looks at 256 of their counts at a time, one per thread
// (a workgroup that walked its rows one dependent load after the other took 20 us to find nothing on 47 891 rows), and lists the
// wide ones in LDS.
__device__ __forceinline__ void order_wide_rows_dealt(const OrderArgs &a, uint32_t block, uint32_t n_blocks) {
    __shared__ uint32_t s_found[ORDER_THREADS], s_n;
    for (uint32_t base = block; base < a.n_rows; base += ORDER_THREADS * n_blocks) {       // (uniform: barriers inside; n_rows < 2^31 task rows)
        const uint64_t p = (uint64_t) base + (uint64_t) threadIdx.x * n_blocks;
        if (threadIdx.x == 0) s_n = 0;
        pdl_sync();
        if (p < a.n_rows && a.row_cnt[p] + (a.mirror_cnt ? a.mirror_cnt[p] : 0u) > ORDER_WAVE_CELLS) s_found[atomicAdd(&s_n, 1u)] = (uint32_t) p;
        pdl_sync();
        const uint32_t n = s_n;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t q = s_found[i], own = a.row_cnt[q];
            order_wide_row(a, q, own, own + (a.mirror_cnt ? a.mirror_cnt[q] : 0u));
        }
        pdl_sync();                              // everybody has read s_n and the list
    }
}
// Rows of at most 256 cells (nearly all rows of most datasets): one wave per row, up to four cells per lane, the keys
// compared through lane reads — no LDS, no barrier, four rows per workgroup.
__global__ __launch_bounds__(256) void k_order_rows_wave(OrderArgs a) {
    const uint32_t p = blockIdx.x * (256 / PDL_WAVE) + threadIdx.x / PDL_WAVE;
    if (p >= a.n_rows) return;
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    const uint32_t own = a.row_cnt[p];
    const uint32_t cnt = own + (a.mirror_cnt ? a.mirror_cnt[p] : 0u);
    if (cnt > ORDER_WAVE_CELLS && lane == 0) *a.wide_rows = 1;       // (plain store of the same value from whoever sees one)
    if (cnt == 0 || cnt > ORDER_WAVE_CELLS) return;      // (wave-uniform)
    const uint32_t nslots = (cnt + PDL_WAVE - 1) / PDL_WAVE;
    uint32_t col[ORDER_CPL], hi_lo[ORDER_CPL], hi_hi[ORDER_CPL], rank[ORDER_CPL];
    OrderCell me[ORDER_CPL];
#pragma unroll
    for (uint32_t s = 0; s < ORDER_CPL; s++) {
        col[s] = 0; hi_lo[s] = 0; hi_hi[s] = 0; rank[s] = 0; me[s] = OrderCell{0, false};
        const uint32_t i = s * PDL_WAVE + lane;
        if (s < nslots && i < cnt) {
            me[s] = order_cell(a, p, own, i);
            const uint2 km = cell_key(a, me[s]);
            col[s] = km.x;
            const unsigned long long hi = order_key_hi(col[s], km.y, a.canonical);
            hi_lo[s] = (uint32_t) hi; hi_hi[s] = (uint32_t) (hi >> 32);
        }
    }
    if (a.pack_ok) {                                     // (uniform) one 64-bit compare per pair instead of a three-word one
        unsigned long long key[ORDER_CPL];
#pragma unroll
        for (uint32_t s = 0; s < ORDER_CPL; s++) {
            const uint32_t i = s * PDL_WAVE + lane;
            key[s] = (s < nslots && i < cnt) ? order_key_packed(col[s], a.canonical ? 0u : hi_lo[s], a.canonical) : ~0ull;
        }
#pragma unroll
        for (uint32_t sj = 0; sj < ORDER_CPL; sj++) {
            if (sj >= nslots) break;
            const uint32_t nj = min((uint32_t) PDL_WAVE, cnt - sj * PDL_WAVE);
            for (uint32_t j = 0; j < nj; j++) {
                const unsigned long long kj = ((unsigned long long) (uint32_t) __shfl((int) (uint32_t) (key[sj] >> 32), (int) j, PDL_WAVE) << 32) |
                                              (uint32_t) __shfl((int) (uint32_t) key[sj], (int) j, PDL_WAVE);
#pragma unroll
                for (uint32_t s = 0; s < ORDER_CPL; s++) rank[s] += kj < key[s] ? 1u : 0u;
            }
        }
    } else
#pragma unroll
    for (uint32_t sj = 0; sj < ORDER_CPL; sj++) {
        if (sj >= nslots) break;
        const uint32_t nj = min((uint32_t) PDL_WAVE, cnt - sj * PDL_WAVE);
        for (uint32_t j = 0; j < nj; j++) {
            const unsigned long long hj = ((unsigned long long) (uint32_t) __shfl((int) hi_hi[sj], (int) j, PDL_WAVE) << 32) |
                                          (uint32_t) __shfl((int) hi_lo[sj], (int) j, PDL_WAVE);
            const uint32_t cj = (uint32_t) __shfl((int) col[sj], (int) j, PDL_WAVE);
#pragma unroll
            for (uint32_t s = 0; s < ORDER_CPL; s++) {
                const unsigned long long hi = ((unsigned long long) hi_hi[s] << 32) | hi_lo[s];
                rank[s] += (hj < hi || (hj == hi && cj < col[s])) ? 1u : 0u;
            }
        }
    }
    const uint32_t out0 = a.fin_off[p];
    const int32_t row = (int32_t) a.task_rows[p];
#pragma unroll
    for (uint32_t s = 0; s < ORDER_CPL; s++) {
        const uint32_t i = s * PDL_WAVE + lane;
        if (s < nslots && i < cnt) {
            const uint32_t o = out0 + rank[s];
            float v_score, v_perc, v_tr;
            cell_values(a, me[s], v_score, v_perc, v_tr);
            a.c_score[o] = v_score; a.c_perc[o] = v_perc; a.c_tr[o] = v_tr;
            a.c_row[o] = row;
            a.c_col[o] = (int32_t) col[s];
        }
    }
}

// Option "order_subwave": a wave ranks 64 / W rows at a time, each in a segment of W lanes (a row of the 64-genome set has ~11
// cells: a whole wave for it keeps a sixth of the lanes busy, and every wave waits through the same chain of dependent loads).
// The rank is the same count over the same keys, read through lane reads of width W; the keys are unique, so where a cell sits
// among the lanes does not matter.  `cnt` is 0 for a segment that sits this call out; `max_cnt` is the largest cnt of the wave
// (uniform): every segment walks that many keys, and what lies behind a row's own cells are padding keys that sort last.
template <uint32_t W>
__device__ __forceinline__ void order_rank_rows(const OrderArgs &a, uint32_t p, uint32_t own, uint32_t cnt, uint32_t sl, uint32_t max_cnt) {
    uint32_t col[ORDER_CPL], first[ORDER_CPL], rank[ORDER_CPL];
    OrderCell me[ORDER_CPL];
#pragma unroll
    for (uint32_t s = 0; s < ORDER_CPL; s++) {
        col[s] = 0xffffffffu; first[s] = 0; rank[s] = 0; me[s] = OrderCell{0, false};
        const uint32_t i = s * W + sl;
        if (i < cnt) {
            me[s] = order_cell(a, p, own, i);
            const uint2 km = cell_key(a, me[s]);
            col[s] = km.x; first[s] = km.y;
        }
    }
    if (a.pack_ok) {                                     // (uniform)
        unsigned long long key[ORDER_CPL];
#pragma unroll
        for (uint32_t s = 0; s < ORDER_CPL; s++) key[s] = s * W + sl < cnt ? order_key_packed(col[s], first[s], a.canonical) : ~0ull;
#pragma unroll
        for (uint32_t sj = 0; sj < ORDER_CPL; sj++) {
            if (sj * W >= max_cnt) break;
            const uint32_t nj = min(W, max_cnt - sj * W);
            for (uint32_t j = 0; j < nj; j++) {
                const unsigned long long kj = ((unsigned long long) (uint32_t) __shfl((int) (uint32_t) (key[sj] >> 32), (int) j, (int) W) << 32) |
                                              (uint32_t) __shfl((int) (uint32_t) key[sj], (int) j, (int) W);
#pragma unroll
                for (uint32_t s = 0; s < ORDER_CPL; s++) rank[s] += kj < key[s] ? 1u : 0u;
            }
        }
    } else {
        unsigned long long hi[ORDER_CPL];                // (a padding cell: every word all ones, behind every key there is)
#pragma unroll
        for (uint32_t s = 0; s < ORDER_CPL; s++) hi[s] = s * W + sl < cnt ? order_key_hi(col[s], first[s], a.canonical) : ~0ull;
#pragma unroll
        for (uint32_t sj = 0; sj < ORDER_CPL; sj++) {
            if (sj * W >= max_cnt) break;
            const uint32_t nj = min(W, max_cnt - sj * W);
            for (uint32_t j = 0; j < nj; j++) {
                const unsigned long long hj = ((unsigned long long) (uint32_t) __shfl((int) (uint32_t) (hi[sj] >> 32), (int) j, (int) W) << 32) |
                                              (uint32_t) __shfl((int) (uint32_t) hi[sj], (int) j, (int) W);
                const uint32_t cj = (uint32_t) __shfl((int) col[sj], (int) j, (int) W);
#pragma unroll
                for (uint32_t s = 0; s < ORDER_CPL; s++) rank[s] += (hj < hi[s] || (hj == hi[s] && cj < col[s])) ? 1u : 0u;
            }
        }
    }
    if (cnt == 0) return;
    const uint32_t out0 = a.fin_off[p];
    const int32_t row = (int32_t) a.task_rows[p];
#pragma unroll
    for (uint32_t s = 0; s < ORDER_CPL; s++) {
        if (s * W + sl < cnt) {
            const uint32_t o = out0 + rank[s];
            float v_score, v_perc, v_tr;
            cell_values(a, me[s], v_score, v_perc, v_tr);
            a.c_score[o] = v_score; a.c_perc[o] = v_perc; a.c_tr[o] = v_tr;
            a.c_row[o] = row;
            a.c_col[o] = (int32_t) col[s];
        }
    }
}
// The first `short_blocks` workgroups: four waves of 64 / W rows each.  A row of up to W x ORDER_CPL cells is ranked in its
// segment; one of more, up to ORDER_WAVE_CELLS, by the whole wave afterwards (uniform: the count comes from a lane read).
// WIDE: the workgroups behind them do k_order_rows' work in the same launch.  They find their rows themselves (a row count
// above ORDER_WAVE_CELLS) and read nothing this launch writes; a set without such a row costs them one pass over the counts.
template <uint32_t W, bool WIDE>
__global__ __launch_bounds__(ORDER_THREADS) void k_order_rows_sub(OrderArgs a, uint32_t short_blocks) {
    static_assert(W == 16 || W == 32, "segments of 16 or 32 lanes");
    if (WIDE && blockIdx.x >= short_blocks) { order_wide_rows_dealt(a, blockIdx.x - short_blocks, gridDim.x - short_blocks); return; }
    constexpr uint32_t R = PDL_WAVE / W, SEG_CELLS = W * ORDER_CPL;
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    const uint32_t p0 = (blockIdx.x * (ORDER_THREADS / PDL_WAVE) + threadIdx.x / PDL_WAVE) * R;       // the wave's first row
    if (p0 >= a.n_rows) return;                          // (wave-uniform)
    const uint32_t p = p0 + lane / W;
    uint32_t own = 0, cnt = 0;
    if (p < a.n_rows) { own = a.row_cnt[p]; cnt = own + (a.mirror_cnt ? a.mirror_cnt[p] : 0u); }
    if (cnt > ORDER_WAVE_CELLS && (lane & (W - 1)) == 0) *a.wide_rows = 1;       // (plain store of the same value from whoever sees one)
    const uint32_t fit = cnt <= SEG_CELLS ? cnt : 0u;
    uint32_t max_cnt = fit;
#pragma unroll
    for (uint32_t d = W; d < PDL_WAVE; d <<= 1) max_cnt = max(max_cnt, (uint32_t) __shfl_xor((int) max_cnt, (int) d, PDL_WAVE));
    if (max_cnt) order_rank_rows<W>(a, p, own, fit, lane & (W - 1), max_cnt);
#pragma unroll
    for (uint32_t s = 0; s < R; s++) {
        const uint32_t cs = (uint32_t) __builtin_amdgcn_readlane((int) cnt, (int) (s * W)), os = (uint32_t) __builtin_amdgcn_readlane((int) own, (int) (s * W));
        if (cs > SEG_CELLS && cs <= ORDER_WAVE_CELLS) order_rank_rows<PDL_WAVE>(a, p0 + s, os, cs, lane, cs);
    }
}

// mirror mode: hand every staged cell (r, c) to row c — as row c reads it: column r, perc and tr_perc swapped — by copying
// it into c's stretch of mcell.  One wave per source row (coalesced reads of its staged cells); the slot inside c's
// stretch is drawn with an atomic (the order inside a stretch is irrelevant: K-order ranks the cells by key).
struct MirrorArgs {
    const uint32_t *row_base, *row_cnt, *task_rows;
    const float *st_score, *st_perc, *st_tr;
    const uint32_t *st_col, *st_first;
    const uint32_t *taskpos_of, *mirror_off;
    uint32_t *mirror_cur;
    uint32_t n_rows;
    MCell *mcell;
};
// source row p, by the W lanes of which this is lane `sl`
template <uint32_t W>
__device__ __forceinline__ void mirror_row(const MirrorArgs &a, uint32_t p, uint32_t sl) {
    const uint32_t base = a.row_base[p], cnt = a.row_cnt[p], r = a.task_rows[p];
    for (uint32_t i = sl; i < cnt; i += W) {
        const uint32_t s = base + i;
        const uint32_t pc = a.taskpos_of[a.st_col[s]];
        if (pc == 0xffffffffu) continue;                 // another GPU's row: the cell travels there (k_outbox)
        const uint32_t dst = a.mirror_off[pc] + atomicAdd(&a.mirror_cur[pc], 1u);
        a.mcell[dst] = MCell{r, a.st_first[s], a.st_score[s], a.st_tr[s], a.st_perc[s], 0u};
    }
}
__global__ __launch_bounds__(256) void k_mirror_cells(MirrorArgs a) {
    const uint32_t p = blockIdx.x * (256 / PDL_WAVE) + threadIdx.x / PDL_WAVE;
    if (p >= a.n_rows) return;
    mirror_row<PDL_WAVE>(a, p, threadIdx.x & (PDL_WAVE - 1));
}
// option "order_subwave": W lanes per source row (a row stages two or three cells of its own on a set of short rows), 256 / W
// rows per workgroup
template <uint32_t W>
__global__ __launch_bounds__(256) void k_mirror_cells_sub(MirrorArgs a) {
    const uint32_t p = blockIdx.x * (256 / W) + threadIdx.x / W;
    if (p >= a.n_rows) return;
    mirror_row<W>(a, p, threadIdx.x & (W - 1));
}

// ------------------------------------------------------------------------------------------------
// Multi-GPU cell exchange.  A staged cell (r, c) whose column c is a row of another GPU is listed for that GPU
// (pdl_dist_cell), grouped by destination: a counting pass and a scattering pass over the staged cells with the same
// rows -> workgroup assignment (LDS counters per destination, no global atomics), an exclusive scan in between.
// The receiver files the cells behind its own staged cells (slot = st_local + i) as mirrored cells of row c.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PDL_MAX_WORLD = 64;
struct OutboxArgs {
    const uint32_t *row_base, *row_cnt, *task_rows;
    const float *st_score, *st_perc, *st_tr;
    const uint32_t *st_col, *st_first;
    const uint32_t *taskpos_of, *genome_of, *owner;
    uint32_t n_rows, rows_per_block, world, n_blocks;
    uint32_t *tab;                 // [world][n_blocks]: counts (pass 1), then their exclusive scan (pass 2 reads `offs`)
    const uint32_t *offs;
    pdl_dist_cell *out;
};
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_outbox(OutboxArgs a) {
    __shared__ uint32_t s_cnt[PDL_MAX_WORLD];
    if (threadIdx.x < PDL_MAX_WORLD) s_cnt[threadIdx.x] = SCATTER && threadIdx.x < a.world ? a.offs[(size_t) threadIdx.x * a.n_blocks + blockIdx.x] : 0u;
    pdl_sync();
    const uint32_t p0 = blockIdx.x * a.rows_per_block, p1 = min(a.n_rows, p0 + a.rows_per_block);
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1);
    for (uint32_t p = p0 + threadIdx.x / PDL_WAVE; p < p1; p += 256 / PDL_WAVE) {
        const uint32_t base = a.row_base[p], cnt = a.row_cnt[p];
        for (uint32_t i = lane; i < cnt; i += PDL_WAVE) {
            const uint32_t col = a.st_col[base + i];
            if (a.taskpos_of[col] != 0xffffffffu) continue;
            const uint32_t d = a.owner[a.genome_of[col]];
            const uint32_t at = atomicAdd(&s_cnt[d], 1u);
            if constexpr (SCATTER)
                a.out[at] = pdl_dist_cell{a.st_score[base + i], a.st_perc[base + i], a.st_tr[base + i], a.task_rows[p], col, a.st_first[base + i]};
        }
    }
    if constexpr (!SCATTER) {
        pdl_sync();
        if (threadIdx.x < a.world) a.tab[(size_t) threadIdx.x * a.n_blocks + blockIdx.x] = s_cnt[threadIdx.x];
    }
}
// first cell of every destination's list + the total, for the host: dst[d] = offs[d][0], dst[world] = total
__global__ void k_outbox_totals(const uint32_t *offs, uint32_t n_blocks, uint32_t world, const uint64_t *d_total, uint32_t *dst) {
    const uint32_t d = threadIdx.x;
    if (d < world) dst[d] = offs[(size_t) d * n_blocks];
    else if (d == world) dst[d] = (uint32_t) *d_total;
}

struct InboxArgs {
    const pdl_dist_cell *in; uint32_t n;
    const uint32_t *taskpos_of, *genome_of, *local_genome;
    uint32_t *mirror_cnt;
    float *MS, *CM;
    uint32_t N, G;
    uint32_t *error_count;
};
// a received cell (r, c): counted for row c and folded into c's maxima (library.cpp:513-515 seen from row c: its column is
// r).  It stays where the exchange put it: k_mirror_cells_inbox copies it from there into c's stretch once the stretches
// are known (it used to be filed in the staging arrays in between: 24 bytes written and read back per cell for nothing).
__global__ __launch_bounds__(256) void k_inbox_file(InboxArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const pdl_dist_cell cl = a.in[i];
    if (cl.column >= a.N || cl.row >= a.N) { atomicAdd(a.error_count, 1u); return; }
    const uint32_t pc = a.taskpos_of[cl.column];
    if (pc == 0xffffffffu) { atomicAdd(a.error_count, 1u); return; }      // not a row of this GPU: the exchange went wrong
    atomicAdd(&a.mirror_cnt[pc], 1u);
    atomicMax(reinterpret_cast<uint32_t *>(a.MS + (size_t) pc * a.G + a.genome_of[cl.row]), __float_as_uint(cl.score));
    atomicMax(reinterpret_cast<uint32_t *>(a.CM + (size_t) a.local_genome[a.genome_of[cl.column]] * a.N + cl.row), __float_as_uint(cl.score));
}
// ... and the cells received from other GPUs (row = the sender's gene)
__global__ __launch_bounds__(256) void k_mirror_cells_inbox(MirrorArgs a, const pdl_dist_cell *__restrict__ in, uint32_t n, uint32_t n_genes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const pdl_dist_cell cl = in[i];
    if (cl.column >= n_genes || cl.row >= n_genes) return;               // (counted as an error by k_inbox_file)
    const uint32_t pc = a.taskpos_of[cl.column];
    if (pc == 0xffffffffu) return;
    const uint32_t dst = a.mirror_off[pc] + atomicAdd(&a.mirror_cur[pc], 1u);
    a.mcell[dst] = MCell{cl.row, cl.first_group, cl.score, cl.tr_perc, cl.perc, 0u};
}

// work-item descriptors of the LDS join, in processing order (currently task order)
// ... and what the join wants to know about a gene when it meets it as a column, gathered into one 16-byte record
struct RowDescArgs {
    const uint32_t *task_rows, *seq_off, *kseq_len, *genome_of, *taskpos_of, *local_genome;
    uint32_t n_rows, n_genes;
    uint4 *desc, *gene_info;
};
__device__ __forceinline__ void row_desc_at(const RowDescArgs &d, uint32_t p) {
    if (p < d.n_genes) {
        const uint32_t g = d.genome_of[p];
        d.gene_info[p] = make_uint4(d.kseq_len[p], g, d.taskpos_of[p], d.local_genome[g]);
    }
    if (p >= d.n_rows) return;
    const uint32_t r = d.task_rows[p];
    const uint32_t e0 = d.seq_off[r];
    d.desc[p] = make_uint4(p, r, e0, d.seq_off[r + 1] - e0);
}
__global__ __launch_bounds__(256) void k_row_desc(RowDescArgs d) { row_desc_at(d, blockIdx.x * 256 + threadIdx.x); }

struct RowCntFlag {
    const uint32_t *row_cnt; const uint32_t *mirror_cnt;     // cells of a row = its own + the mirrored ones
    __device__ uint32_t operator()(uint64_t p) const { return row_cnt[p] + (mirror_cnt ? mirror_cnt[p] : 0u); }
};
struct MirrorCntFlag {
    const uint32_t *mirror_cnt;
    __device__ uint32_t operator()(uint64_t p) const { return mirror_cnt[p]; }
};
struct FinOffApply {
    uint32_t *fin_off;
    __device__ void operator()(uint64_t p, uint32_t, uint32_t prefix) const { fin_off[p] = prefix; }
};
// K-order's offsets in ONE launch (mirror mode, up to OO_MAX_ROWS rows): fin_off[p] = cells (own + mirrored) of the rows before
// p, m_off[p] = their mirrored cells, and the two totals — what scan_and_apply(RowCntFlag) + scan_and_apply(MirrorCntFlag) make
// in four dependent launches that are nearly all launch cost at these sizes.  Both prefixes ride in one u64 (cells << 32 |
// mirrored: each total stays below 2^32, nothing carries across).  A workgroup owns `span` rows (a multiple of OO_TILE; one
// workgroup: all of them): it adds up the raw counts in front of its part itself (L2-resident, at most 2 x 4 x OO_MAX_ROWS bytes),
// then scans its part OO_TILE rows at a time, four consecutive rows per thread.  Nobody waits for another workgroup.
constexpr uint32_t OO_THREADS = 1024, OO_ITEMS = 4, OO_TILE = OO_THREADS * OO_ITEMS;
// The bound: the last workgroup reads all counts in front of it, 1 MiB at 2^17 rows — about 7 us from L2 for one CU, half of
// the three launches the kernel saves; beyond it the scans' parallel tiles are the better tool.
constexpr uint32_t OO_MAX_ROWS = 1u << 17;
__device__ __forceinline__ unsigned long long oo_pack(uint32_t cells, uint32_t mirrored) { return ((unsigned long long) cells << 32) + mirrored; }
// exclusive prefix of v over the workgroup's OO_THREADS threads, the workgroup's sum in `total`; `extra` is added up over the
// workgroup behind the same barriers (extra_total)
__device__ __forceinline__ unsigned long long oo_block_scan(unsigned long long v, unsigned long long extra, unsigned long long *s_wave /* [17] */,
                                                            unsigned long long *s_extra /* [16] */, unsigned long long &total, unsigned long long &extra_total) {
    constexpr uint32_t NW = OO_THREADS / PDL_WAVE;
    const uint32_t lane = threadIdx.x & (PDL_WAVE - 1), wave = threadIdx.x / PDL_WAVE;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < PDL_WAVE; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, PDL_WAVE);
        if (lane >= (uint32_t) d) inc += o;
    }
#pragma unroll
    for (int d = PDL_WAVE / 2; d > 0; d >>= 1) extra += __shfl_xor(extra, d, PDL_WAVE);
    if (lane == PDL_WAVE - 1) { s_wave[wave] = inc; s_extra[wave] = extra; }
    pdl_sync();
    if (threadIdx.x < PDL_WAVE) {                            // (the first wave, whole: the 16 wave sums)
        const unsigned long long w = lane < NW ? s_wave[lane] : 0ull;
        unsigned long long winc = w, e = lane < NW ? s_extra[lane] : 0ull;
#pragma unroll
        for (int d = 1; d < (int) NW; d <<= 1) {
            const unsigned long long o = __shfl_up(winc, d, PDL_WAVE);
            if (lane >= (uint32_t) d) winc += o;
        }
#pragma unroll
        for (int d = (int) NW / 2; d > 0; d >>= 1) e += __shfl_xor(e, d, PDL_WAVE);
        if (lane < NW) s_wave[lane] = winc - w;
        if (lane == NW - 1) s_wave[16] = winc;
        if (lane == 0) s_extra[0] = e;
    }
    pdl_sync();
    const unsigned long long res = inc - v + s_wave[wave];
    total = s_wave[16]; extra_total = s_extra[0];
    pdl_sync();
    return res;
}
__global__ __launch_bounds__(OO_THREADS) void k_order_offsets(const uint32_t *__restrict__ row_cnt, const uint32_t *__restrict__ mirror_cnt, uint32_t n_rows,
                                                              uint32_t span, uint32_t *__restrict__ fin_off, uint32_t *__restrict__ m_off,
                                                              uint64_t *d_emitted, uint64_t *d_mirrored) {
    __shared__ unsigned long long s_wave[17], s_extra[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t r0 = min(blockIdx.x * span, n_rows), r1 = min(r0 + span, n_rows);
    unsigned long long carry = 0;                            // cells | mirrored cells of the rows before the current trip
    for (uint32_t base = r0; base < r1; base += OO_TILE) {   // (uniform: barriers inside)
        const uint32_t i0 = base + tid * OO_ITEMS;
        const bool whole = i0 + OO_ITEMS <= r1;              // (16-byte loads: both arrays start an allocation, i0 is a multiple of four)
        uint32_t f[OO_ITEMS], m[OO_ITEMS];
        if (whole) {
            const uint4 rc = *reinterpret_cast<const uint4 *>(row_cnt + i0), mc = *reinterpret_cast<const uint4 *>(mirror_cnt + i0);
            m[0] = mc.x; m[1] = mc.y; m[2] = mc.z; m[3] = mc.w;
            f[0] = rc.x + mc.x; f[1] = rc.y + mc.y; f[2] = rc.z + mc.z; f[3] = rc.w + mc.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < OO_ITEMS; j++) {
                const bool live = i0 + j < r1;
                m[j] = live ? mirror_cnt[i0 + j] : 0u;
                f[j] = live ? row_cnt[i0 + j] + m[j] : 0u;
            }
        }
        // first trip: the rows in front of the part, 16 bytes a load and sixteen loads in flight per thread (one load at a time,
        // each waited for, took 19 us for 45 000 rows: latency, not bytes); 32-bit sums: the totals stay below 2^32
        uint32_t pc = 0, pm = 0;
        if (base == r0) {
            const uint32_t n4 = r0 / 4;                      // (r0 is a multiple of four: span is one of OO_TILE)
            const uint4 *rc4 = reinterpret_cast<const uint4 *>(row_cnt), *mc4 = reinterpret_cast<const uint4 *>(mirror_cnt);
#pragma unroll 8
            for (uint32_t i = tid; i < n4; i += OO_THREADS) {
                const uint4 a = rc4[i], b = mc4[i];
                pc += a.x + a.y + a.z + a.w; pm += b.x + b.y + b.z + b.w;
            }
        }
        unsigned long long sum = 0, total, front;
#pragma unroll
        for (uint32_t j = 0; j < OO_ITEMS; j++) sum += oo_pack(f[j], m[j]);
        unsigned long long ex = oo_block_scan(sum, oo_pack(pc + pm, pm), s_wave, s_extra, total, front);
        carry += front;
        ex += carry;
#pragma unroll
        for (uint32_t j = 0; j < OO_ITEMS; j++) {
            if (i0 + j < r1) { fin_off[i0 + j] = (uint32_t) (ex >> 32); m_off[i0 + j] = (uint32_t) ex; }
            ex += oo_pack(f[j], m[j]);
        }
        carry += total;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {           // the last part ends the rows: its carry is the totals
        const uint32_t cells = (uint32_t) (carry >> 32);
        *d_emitted = cells;
        fin_off[n_rows] = cells; fin_off[n_rows + 1] = 0u;   // (the total closes fin_off; written as a u64 in two words, as the scan does)
        *d_mirrored = (uint32_t) carry;
    }
}

// dst[0..n) = src[idx[..]]; then the join counters and the emitted-cell total (u64 as two words) are appended (PDL_JT_*), so
// the host fetches everything it wants to know after a scoring pass with ONE copy
__global__ void k_gather_u32(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t *dst, const uint32_t *ctr, const uint32_t *z64) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
    else if (i < n + PDL_JT_CTR_WORDS) dst[i] = ctr[i - n];
    else if (i < n + PDL_JT_EMITTED + 2) dst[i] = z64[i - n - PDL_JT_EMITTED];
    else if (i == n + PDL_JT_RELOADS) dst[i] = ctr[PDL_JC_RELOADS];
    else if (i == n + PDL_JT_ROWS_T1) dst[i] = ctr[PDL_JC_ROWS_T1];
}

// Clears up to four arrays in one launch (16-byte words; every separate small fill is a dispatch of its own).
struct ZeroRanges { uint4 *p[4]; unsigned long long n16[4]; };
__device__ __forceinline__ void zero_ranges_by(const ZeroRanges &z, uint32_t block, uint32_t n_blocks) {
    const unsigned long long stride = (unsigned long long) n_blocks * 256;
#pragma unroll
    for (int r = 0; r < 4; r++)
        for (unsigned long long i = (unsigned long long) block * 256 + threadIdx.x; i < z.n16[r]; i += stride) z.p[r][i] = make_uint4(0, 0, 0, 0);
}
__global__ __launch_bounds__(256) void k_zero_ranges(ZeroRanges z) { zero_ranges_by(z, blockIdx.x, gridDim.x); }
// Option "fused_glue": what opens the first scoring pass over a task layout in ONE launch — the first `desc_blocks` workgroups
// write the row and gene descriptors, the ones behind them clear.  Neither half reads or writes what the other touches.
__global__ __launch_bounds__(256) void k_open_pass(RowDescArgs d, ZeroRanges z, uint32_t desc_blocks) {
    if (blockIdx.x < desc_blocks) row_desc_at(d, blockIdx.x * 256 + threadIdx.x);
    else zero_ranges_by(z, blockIdx.x - desc_blocks, gridDim.x - desc_blocks);
}

// ------------------------------------------------------------------------------------------------
// Task layout of the shard on the host and its upload: shard genomes ascending, rows of a genome ascending
// (library.cpp:244).  Called from the preprocess while the device is busy sorting, and again only if the shard
// changed since.  The host vectors live in the context, so the asynchronous copies need no synchronisation here.
void pdl_prepare_tasks(pdl_ctx *c) {
    hipStream_t st = c->stream;
    const uint32_t N = c->N, G = c->G;
    if (!c->shard_set) { c->shard.resize(G); for (uint32_t g = 0; g < G; g++) c->shard[g] = g; }
    const uint32_t S = (uint32_t) c->shard.size();
    c->h_local_genome.assign(G, -1);
    c->h_task_row_off.assign(S + 1, 0);
    uint32_t n_rows = 0;
    for (uint32_t i = 0; i < S; i++) n_rows += c->h_genome_row_off[c->shard[i] + 1] - c->h_genome_row_off[c->shard[i]];
    // one pinned staging buffer, filled in place: task_rows[n_rows] | task_lg[n_rows] | taskpos_of[N] | local_genome[G]
    // -> ONE upload (separate copies from pageable vectors were five staged transfers with the device idle in between)
    const size_t words = 2 * (size_t) n_rows + N + G;
    const size_t words_all = words + S + 1;                  // ... | task_row_off[S + 1] (goes to its own buffer)
    if (c->task_pin_words < words_all) {
        if (c->task_pin) (void) hipHostFree(c->task_pin);
        c->task_pin = nullptr; c->task_pin_words = 0;
        PDL_HIP(hipHostMalloc((void **) &c->task_pin, (words_all + words_all / 4 + 16) * sizeof(uint32_t), hipHostMallocDefault));
        c->task_pin_words = words_all + words_all / 4 + 16;
    }
    uint32_t *h_rows = c->task_pin, *h_lg = h_rows + n_rows, *h_pos = h_lg + n_rows, *h_loc = h_pos + N;
    for (uint32_t i = 0; i < N; i++) h_pos[i] = 0xffffffffu;
    uint32_t p = 0;
    for (uint32_t i = 0; i < S; i++) {
        const uint32_t g = c->shard[i];
        c->h_local_genome[g] = (int32_t) i;
        c->h_task_row_off[i] = p;
        for (uint32_t j = c->h_genome_row_off[g]; j < c->h_genome_row_off[g + 1]; j++) { const uint32_t gene = c->h_genome_rows[j]; h_rows[p] = gene; h_lg[p] = i; h_pos[gene] = p; p++; }
    }
    for (uint32_t g = 0; g < G; g++) h_loc[g] = (uint32_t) c->h_local_genome[g];       // (int32 -1 reads as 0xffffffff)
    c->h_task_row_off[S] = n_rows;
    c->n_task_rows = n_rows;
    c->tasks_ready = true;
    // The uploads travel on a stream of their own: a copy queued between two kernels of the build costs ~10 us of idle
    // stream on either side (the blit's barrier packets) — here the build's kernels go on undisturbed and the main stream
    // waits for the event, which has long fired when the first kernel that reads the task layout comes up.
    if (!c->copy_stream) {
        PDL_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        PDL_HIP(hipEventCreateWithFlags(&c->ev_tasks, hipEventDisableTiming));
    }
    memcpy(c->task_pin + words, c->h_task_row_off.data(), (size_t) (S + 1) * 4);
    c->task_blob.alloc(words * sizeof(uint32_t) + 16);
    if (n_rows) c->task_off.alloc((size_t) (S + 1) * 8 + 96);      // task offsets | gathered cell offsets + PDL_JT_WORDS counters (and room to spare)
    PDL_HIP(hipMemcpyAsync(c->task_blob.p, c->task_pin, words * sizeof(uint32_t), hipMemcpyHostToDevice, c->copy_stream));
    if (n_rows) PDL_HIP(hipMemcpyAsync(c->task_off.p, c->task_pin + words, (size_t) (S + 1) * 4, hipMemcpyHostToDevice, c->copy_stream));
    PDL_HIP(hipEventRecord(c->ev_tasks, c->copy_stream));
    PDL_HIP(hipStreamWaitEvent(st, c->ev_tasks, 0));
    uint32_t *d = c->task_blob.as<uint32_t>();
    c->task_rows.p = d; c->task_lg.p = d + n_rows; c->taskpos_of.p = d + 2 * (size_t) n_rows; c->local_genome.p = d + 2 * (size_t) n_rows + N;
    if (c->dist) {            // genome -> rank, for the cell exchange
        c->owner_of_genome.alloc((size_t) G * 4);
        PDL_HIP(hipMemcpyAsync(c->owner_of_genome.p, c->h_owner.data(), (size_t) G * 4, hipMemcpyHostToDevice, st));
    }
}

__global__ void k_iota_u32(uint32_t *dst, uint32_t n) { uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) dst[i] = i; }

// ------------------------------------------------------------------------------------------------
// The scoring pass on the host: plan (sizes, tiers), join (the tiers queued back to back), then the
// emission-order pass.  Single GPU: join + order, the host looks at the counters once, at the end; a staging area
// that turns out too small repeats the pass once with the size asked for (rows that did not fit hold no cell, so
// everything queued behind an overflowing join stays inside its buffers).  Multi-GPU: join + outbox listing
// (pdl_dist_score_begin), the caller's all-to-all, inbox filing + order (pdl_dist_score_finish).
// ------------------------------------------------------------------------------------------------

// The tier table: every instance of the join kernels the host launches, by tier and form, with its workgroup size.  The
// occupancy query and the launch both go through an entry; pdl_ctx::join_occ caches the occupancy by entry.
//   0  k_join_part            short rows, several per workgroup cycle (0B: 512 threads, for the rows that alone exceed that cycle)
//   1  k_join_lds<FILTER>     small table + "seen twice" bitmap, several rows resident per CU
//   2  k_join_lds<13,1024>    128-KiB table holding every column a row touches, one row per CU
//   3  k_join_hbm             direct-addressed tables in HBM
enum JoinTier { TIER0, TIER0B, TIER1, TIER2, TIER3 };
struct JoinKernel { JoinTier tier; int form; void (*fn)(JoinArgs); uint32_t threads; };
static const JoinKernel JOIN_KERNELS[] = {
    {TIER0, 0, k_join_part<PT_T, PT_WG_PER_CU, false>, PT_T}, {TIER0, 1, k_join_part<PT_T, PT_WG_PER_CU, true>, PT_T},       // form: the sift has counters
    {TIER0B, 0, k_join_part<PT_T2, PT_WGS2, false>, PT_T2},   {TIER0B, 1, k_join_part<PT_T2, PT_WGS2, true>, PT_T2},
    {TIER1, 9, k_join_lds<9, 128, true>, 128}, {TIER1, 10, k_join_lds<10, 256, true>, 256}, {TIER1, 11, k_join_lds<11, 256, true>, 256},      // form: "join_tier1"
    {TIER1, 20, k_join_lds<10, 256, false>, 256}, {TIER1, 21, k_join_lds<11, 256, false>, 256},
    {TIER2, 0, k_join_lds<13, 1024, false>, 1024}, {TIER2, 1, k_join_lds<9, 64, false>, 64},                                  // form: "join_tiny_tier2"
    {TIER3, 0, k_join_hbm<false>, HBM_THREADS},    {TIER3, 1, k_join_hbm<true>, HBM_THREADS},                                 // form: 32-bit counters
};
static int join_kernel(JoinTier tier, int form) {
    for (int i = 0; i < (int) (sizeof(JOIN_KERNELS) / sizeof(JoinKernel)); i++) if (JOIN_KERNELS[i].tier == tier && JOIN_KERNELS[i].form == form) return i;
    PDL_FAIL(PDL_ERR_STATE, "join: no kernel for tier %d in form %d", (int) tier, form);
}
static uint32_t join_occupancy(pdl_ctx *c, int kernel) {
    static_assert(sizeof(JOIN_KERNELS) / sizeof(JoinKernel) <= sizeof(pdl_ctx::join_occ) / sizeof(uint32_t), "pdl_ctx::join_occ holds every entry");
    int nb = (int) c->join_occ[kernel];
    if (nb == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *) JOIN_KERNELS[kernel].fn, (int) JOIN_KERNELS[kernel].threads, 0) != hipSuccess || nb < 1)) nb = 1;
    return c->join_occ[kernel] = (uint32_t) nb;
}

// tier 3's tables in glb_table: the sums of every workgroup (u64 [N]; with 32-bit counters u32 [3][N] in twice the bytes), and
// behind the sums of ALL workgroups their first / touched / emit lists (u32 [N] each)
struct HbmLayout { size_t sums, lists; size_t per_wg() const { return sums + lists; } };      // bytes per workgroup
static HbmLayout hbm_layout(uint32_t N, bool wide) { return {(size_t) N * (wide ? 2 : 1) * sizeof(uint64_t), (size_t) N * 3 * sizeof(uint32_t)}; }

struct ScorePlan {
    bool wide, mirror;
    bool tier0;                    // the partition tier runs in front of tier 1 (short rows)
    int tier1;                     // "join_tier1": the tier-1 table (0: no tier 1)
    int k0, k0b, k1, k2, k3;       // the tiers' entries of the table (k0, k0b: with tier0; k1: with tier1)
    uint32_t grid0, grid0b;        // (the second form of the partition tier: 512 threads, the rows that alone exceed the first form's cycle)
    uint32_t grid1, grid2, grid3;
    unsigned long long slack;
    bool wide_aside;               // put-aside entries carry row and launch in full (16 bytes): gene ids beyond 22 bits, or the repeat of a pass
                                   // whose 10-bit tags saw an entry that had to be loaded again
};

static ScorePlan score_plan(pdl_ctx *c) {
    const uint32_t N = c->N, G = c->G;
    const uint32_t n_rows = c->n_task_rows;
    const uint32_t S = (uint32_t) c->shard.size();
    ScorePlan pl{};
    // the LDS tiers pack the three sums of a cell in 21-bit fields; a gene with >= 2^20 k-mers could overflow them, so
    // such a dataset is scored entirely by the HBM kernel with 32-bit counters (the reference's ints)
    pl.wide = c->max_kseq >= (1ull << 20);
    if (c->max_kseq >= (1ull << 31)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "a gene with %llu k-mers exceeds the reference's int counters", (unsigned long long) c->max_kseq);
    // mirror mode (ranges hold only the genes above the row): every staged cell (r, c) is also cell (c, r)
    pl.mirror = c->upper_only;
    if (pl.mirror && !c->dist && (c->shard_set && S != G))
        PDL_FAIL(PDL_ERR_STATE, "the dictionary was built for all genomes (upper-triangle ranges); a genome shard must be set before pdl_preprocess");
    const int cus = pdl_cus(c);
    // ---- tiers (the table above) ------------------------------------------------------------------------
    // A tier hands the rows it cannot hold to the next one through a device-side list.  pdl_set_option "join_tier1"
    // picks the tier-1 table (0: skip tier 1; 20 / 21: 1024 / 2048-slot tables WITHOUT the filter, one pass);
    // "join_tiny_tier2" swaps tier 2 for a tiny table so that tests can reach tier 3 with small inputs.
    pl.tier1 = c->opt_tier1 >= 0 ? c->opt_tier1 : (G <= 320 ? 10 : 11);    // keys per row ~ homologs (about one per genome) + repeated/colliding noise
    const int tier1 = pl.tier1;
    pl.k1 = tier1 ? join_kernel(TIER1, tier1) : -1; pl.k2 = join_kernel(TIER2, c->opt_tiny_tier2); pl.k3 = join_kernel(TIER3, pl.wide);
    pl.grid1 = tier1 ? std::min<uint32_t>(n_rows, (uint32_t) cus * join_occupancy(c, pl.k1)) : 0;
    if (c->opt_grid_pct > 0 && pl.grid1) pl.grid1 = std::max<uint32_t>(1, (uint32_t) ((uint64_t) pl.grid1 * (uint32_t) c->opt_grid_pct / 100));     // (experiments: fewer rows in flight)
    // tier 0, the partition tier: packed ranges (gene ids below 2^22), no gene of <= 2k k-mers (single sightings are never
    // emitted), short rows on average (a cycle takes 4096 lookups: rows of several thousand would all be handed on).
    // "join_tier0" 1 / 0 forces it on / off; choosing the tier-1 table by hand ("join_tier1") leaves it off unless forced.
    {
        const unsigned long long walked = c->dist ? [&] { unsigned long long u = 0; for (uint32_t g : c->shard) u += c->h_upper_cost[g]; return u; }()
                                          : pl.mirror ? (c->P - c->Ushared) / 2 : c->P;
        const bool can = c->ranges8 != nullptr && !pl.wide && c->min_kseq > 2ull * c->rp.k && tier1 != 0;
        // by itself only where it has paid on every set measured: short rows (a cycle holds 4096 lookups) of genes whose k-mers
        // rarely repeat inside the gene — low-complexity stretches make rows wide and their lookups heavy, and such rows are handed
        // on after the work was done (protein-like stand-in: 1.05 ms with this tier in front, 0.64 without)
        const bool want = c->opt_tier0 > 0 || (c->opt_tier0 < 0 && c->opt_tier1 < 0 && n_rows >= 12288 && walked / n_rows <= 3000 && c->Urepeat * 5000 <= c->U);      // (fewer rows: the extra launches cost more than the tier saves)
        pl.tier0 = can && want;
        if (pl.tier0) {
            // the sift: counters against the set's threshold clamp(tc_min, 2, 255) (the kernel works it out the same way) where that is
            // high enough for 12 index bits to beat "seen twice" on 15 (PT_SIFT_T_MIN), bitmaps below it.  "sift_threshold" 0 is the test
            // switch: the counters at a threshold of 2, whatever the set's.
            const uint32_t t = min_numerator(1.0f / (2.0f * (float) c->rp.k), (float) (int) (uint32_t) std::max<uint64_t>(c->min_kseq, 1));
            const bool counters = c->opt_sift_threshold == 0 || t >= PT_SIFT_T_MIN;
            pl.k0 = join_kernel(TIER0, counters); pl.k0b = join_kernel(TIER0B, counters);
            pl.grid0 = std::min<uint32_t>((n_rows + PT_BATCH - 1) / PT_BATCH, (uint32_t) cus * join_occupancy(c, pl.k0));
            pl.grid0b = std::min<uint32_t>(n_rows, (uint32_t) cus * join_occupancy(c, pl.k0b));
            if (c->opt_grid_pct > 0) pl.grid0 = std::max<uint32_t>(1, (uint32_t) ((uint64_t) pl.grid0 * (uint32_t) c->opt_grid_pct / 100));
        }
    }
    pl.grid2 = std::min<uint32_t>(n_rows, (uint32_t) cus * (c->opt_tiny_tier2 ? 4 : 1));
    // tier 3: a direct-addressed table per workgroup (20 bytes per gene; 28 with 32-bit counters): as many workgroups as ~8 GB
    // of tables allow, at least 64 (configs[4]: 2 778 rows of the first genomes end up here, 0.6 ms each — 64 workgroups took
    // 26.7 ms over them)
    const unsigned long long fit = ((c->opt_low_memory ? 1ull : 8ull) << 30) / hbm_layout(std::max<uint32_t>(N, 1), pl.wide).per_wg();
    pl.grid3 = (uint32_t) std::min<unsigned long long>((unsigned long long) cus, std::max<unsigned long long>(64, fit));
    const size_t hbm_bytes = (size_t) pl.grid3 * hbm_layout(N, pl.wide).per_wg();
    if (c->glb_table.bytes < hbm_bytes) { c->glb_table.alloc(hbm_bytes); c->glb_clean = false; }
    // k_join_hbm leaves its tables zeroed, not its touched / emitted lists, and the workgroups' tables and lists are laid out by N,
    // the workgroup count and the counter width: a context rebuilt on a set of another size finds the old lists where its tables
    // are.  One memset per allocation AND per layout (as q_join_hbm_tier keeps it for the query's tables).
    if (c->glb_cols != N || c->glb_slots != pl.grid3 || c->glb_wide != pl.wide) c->glb_clean = false;
    if (!c->glb_clean) {
        PDL_HIP(hipMemsetAsync(c->glb_table.p, 0, hbm_bytes, c->stream));
        c->glb_clean = true;
    }
    c->glb_cols = N; c->glb_slots = pl.grid3; c->glb_wide = pl.wide;
    // Every workgroup reserves staging in chunks of CELL_CHUNK cells: a partly used chunk per workgroup of every tier
    pl.slack = 2ull * (pl.grid0 + pl.grid0b + pl.grid1 + pl.grid2 + pl.grid3) * CELL_CHUNK;
    return pl;
}

// The hand-over from tier to tier.  A tier draws its work with a cursor word of join_ctr, `batch` items a draw: every row (row_desc;
// the host knows how many) or what the tier in front listed in a link.  A link is a count word of join_ctr, one of the row lists of
// overflow_rows (task positions) and one of the descriptor lists of row_desc2: a tier writes the descriptors of the rows it hands
// on beside their positions, so the reader starts without a pass that makes them.  Tier 3 alone goes by the task positions.
struct JoinLink { uint32_t count, cursor, rows; int desc; };      // PDL_JC_* of the count and of the reader's cursor | row list | descriptor list (-1: none)
constexpr JoinLink LINK_T1_T2{PDL_JC_ROWS_T2, PDL_JC_CURSOR_T2, 0, 0}, LINK_T2_T3{PDL_JC_ROWS_T3, PDL_JC_CURSOR_T3, 1, -1},
                   LINK_T0_T0B{PDL_JC_ROWS_T0B, PDL_JC_CURSOR_T0B, 2, 1}, LINK_T0B_T1{PDL_JC_ROWS_T1, PDL_JC_CURSOR_T1, 3, 2};
constexpr uint32_t JOIN_ROW_LISTS = 4, JOIN_DESC_LISTS = 3;       // (n_task_rows entries each)
struct TierIn { const uint4 *desc; const uint32_t *work; uint32_t n; const uint32_t *n_ptr; uint32_t *cursor; uint32_t batch; };      // descriptors or task positions | host or device count
struct TierOut { uint32_t *count, *rows; uint4 *desc; };
struct JoinLists {
    uint32_t *ctr, *rows; uint4 *desc; const uint4 *all_desc; uint32_t n_rows, n_all;      // n_all: 0 when the whole set goes to tier 3 (the LDS tiers still launch, and leave at once)
    TierOut out(const JoinLink &l) const { return {ctr + l.count, rows + (size_t) l.rows * n_rows, l.desc < 0 ? nullptr : desc + (size_t) l.desc * n_rows}; }
    TierIn in(const JoinLink &l) const { const TierOut o = out(l); return {o.desc, o.desc ? nullptr : o.rows, 0, o.count, ctr + l.cursor, 1}; }      // (few, long rows: one a draw)
    TierIn all(uint32_t cursor_word, uint32_t batch) const { return {all_desc, nullptr, n_all, nullptr, ctr + cursor_word, batch}; }
    TierIn spread(uint32_t cursor_word, uint32_t grid) const { return all(cursor_word, std::max<uint32_t>(1, std::min<uint32_t>(8, n_rows / (std::max<uint32_t>(grid, 1) * 8)))); }      // (up to 8 a draw while every workgroup gets 8 draws)
};

// One tier: an entry of the table at `grid` workgroups, reading `in` and handing on through `out`.  `timed` counts in the diagnostic
// build (-DPDL_JOIN_PHASES) only: the kernel's phase words are cleared in front of the launch and printed behind it (which waits for the
// stream), n_timers as us per workgroup — thread 0's clock, waiting for every access it brackets: read the shares, not the sum — then counts.
struct TierPhases { const char *tier; uint32_t n_timers, n_words; const char *label[12]; };
static const TierPhases PHASES_T0{"tier 0", 6, 12, {"draw + pick", "stage", "prefixes", "walk", "sift + add", "finalize", "cycles", "cycles that overflowed",
                                                     "survivors of wave 0 (x4 for all)", "probe steps of thread 0", "lookups", "rows"}},
                        PHASES_T1{"tier 1", 10, 10, {"dispense", "stage", "barrier", "aside pass", "finalize", "walk: map", "postings", "bitmap", "table", "aside stores"}};
static void launch_tier(pdl_ctx *c, JoinArgs a, int kernel, uint32_t grid, const TierIn &in, const TierOut &out, const TierPhases *timed = nullptr) {
    a.desc = in.desc; a.work = in.work; a.n_work = in.n; a.n_work_ptr = in.n_ptr; a.work_cursor = in.cursor; a.work_batch = in.batch;
    a.overflow_count = out.count; a.overflow_rows = out.rows; a.overflow_desc = out.desc;
#ifdef PDL_JOIN_PHASES
    static unsigned long long *d_phase = nullptr;
    unsigned long long h[12];
    if (timed && !d_phase) PDL_HIP(hipMalloc((void **) &d_phase, sizeof(h)));
    if (timed) { PDL_HIP(hipMemsetAsync(d_phase, 0, sizeof(h), c->stream)); a.phase = d_phase; }
#endif
    hipLaunchKernelGGL(JOIN_KERNELS[kernel].fn, dim3(grid), dim3(JOIN_KERNELS[kernel].threads), 0, c->stream, a);
#ifdef PDL_JOIN_PHASES
    if (!timed) return;
    PDL_HIP(hipMemcpyAsync(h, d_phase, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PDL_HIP(hipStreamSynchronize(c->stream));
    const double wgs = std::max<uint32_t>(grid, 1);
    fprintf(stderr, "%s, phases per workgroup (us) and counts:", timed->tier);
    for (uint32_t i = 0; i < timed->n_words; i++)
        if (i < timed->n_timers) fprintf(stderr, "  %s %.1f", timed->label[i], h[i] * (10.0 / 1000.0) / wgs);      // (ticks of 10 ns)
        else fprintf(stderr, "  %s %llu", timed->label[i], h[i]);
    fprintf(stderr, "  | rows/wg %.1f\n", (double) c->n_task_rows / wgs);
#endif
}

static RowDescArgs row_desc_args(pdl_ctx *c) {
    return {c->task_rows.as<uint32_t>(), c->seq_off.as<uint32_t>(), c->kseq_len.as<uint32_t>(), c->d_gen, c->taskpos_of.as<uint32_t>(), c->local_genome.as<uint32_t>(),
            c->n_task_rows, c->N, c->row_desc.as<uint4>(), c->gene_info.as<uint4>()};
}
static uint32_t row_desc_blocks(const pdl_ctx *c) { return (std::max(c->n_task_rows, c->N) + 255) / 256; }

// buffers that depend on the row count only
static void score_alloc_rows(pdl_ctx *c, const ScorePlan &pl) {
    const uint32_t N = c->N, G = c->G, n_rows = c->n_task_rows;
    const uint32_t S = (uint32_t) c->shard.size();
    c->MS.alloc((size_t) n_rows * G * sizeof(float) + 16);      // (+16: cleared in whole 16-byte words)
    c->CM.alloc((size_t) S * N * sizeof(float) + 16);
    c->row_base.alloc((size_t) n_rows * 4); c->row_cnt.alloc((size_t) n_rows * 4); c->fin_off.alloc(((size_t) n_rows + 2) * 4);      // (+1: the scan stores its 64-bit total at [n_rows])
    c->join_ctr.alloc(PDL_JC_WORDS * sizeof(uint32_t));
    c->row_desc.alloc((size_t) n_rows * sizeof(uint4));
    c->row_desc2.alloc((size_t) n_rows * sizeof(uint4) * (pl.tier0 ? JOIN_DESC_LISTS : 1));      // (the links of tier 0 come last)
    c->overflow_rows.alloc((size_t) n_rows * 4 * JOIN_ROW_LISTS);
    if (pl.mirror) c->mirror_cnt.alloc((size_t) n_rows * 4 * 3 + 16);    // counts | offsets | cursors
    c->gene_info.alloc((size_t) N * sizeof(uint4));
    // the descriptors: with the clearing launch of the first pass (option "fused_glue"), or here
    if (!c->opt_fused_glue) hipLaunchKernelGGL(k_row_desc, dim3(row_desc_blocks(c)), dim3(256), 0, c->stream, row_desc_args(c));
}

// staging for `cap` cells of this context's rows; final cells and mirrored copies also for `extra` cells received from other
// GPUs (those stay in the caller's exchange buffer until they are copied into their rows' stretches).  Growing `extra` after
// the join leaves the staged cells alone: the staging arrays already have their size.
static void score_alloc_cells(pdl_ctx *c, const ScorePlan &pl, unsigned long long cap, unsigned long long extra) {
    const unsigned long long fcap = pl.mirror ? 2 * cap + extra : cap;          // final cells: staged ones + their mirrors + received ones
    if (fcap >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 emitted cells on one device: shard the genomes over more devices");
    DevBuf *st[5] = {&c->st_score, &c->st_perc, &c->st_tr, &c->st_col, &c->st_first};
    for (int i = 0; i < 5; i++) st[i]->alloc(cap * 4);
    c->c_score.alloc(fcap * 4); c->c_perc.alloc(fcap * 4); c->c_tr.alloc(fcap * 4); c->c_row.alloc(fcap * 4); c->c_col.alloc(fcap * 4);
    if (pl.mirror) c->mirror_ref.alloc((cap + extra) * sizeof(MCell));     // the mirrored cells, copied (one per staged / received cell)
    c->st_cap = cap;
}

// The staged cells of a pass — where a row's cells start, how many it has, whose row it is, and the five staging arrays — as
// JoinArgs, MirrorArgs, OrderArgs and OutboxArgs all name them: one fill for whichever of those is in hand.
struct StagedCells { uint32_t *row_base, *row_cnt; const uint32_t *task_rows; float *st_score, *st_perc, *st_tr; uint32_t *st_col, *st_first; };
static StagedCells staged_cells(pdl_ctx *c) {
    return {c->row_base.as<uint32_t>(), c->row_cnt.as<uint32_t>(), c->task_rows.as<uint32_t>(), c->st_score.as<float>(), c->st_perc.as<float>(), c->st_tr.as<float>(), c->st_col.as<uint32_t>(), c->st_first.as<uint32_t>()};
}
template <class Args> static void set_staged_cells(Args &a, const StagedCells &s) {
    a.row_base = s.row_base; a.row_cnt = s.row_cnt; a.task_rows = s.task_rows;
    a.st_score = s.st_score; a.st_perc = s.st_perc; a.st_tr = s.st_tr; a.st_col = s.st_col; a.st_first = s.st_first;
}

// K-order's kernels: rows of up to 256 cells inside a wave or a segment of one, and the rows that are left for the workgroup
// kernel, if any.  Option "order_subwave" (W lanes per short row; 1: ORDER_SUB_W) puts both into one launch unless
// "order_wide_merged" is 0; "order_subwave" 0: a wave per short row, and k_order_rows behind it.
template <uint32_t W>
static void launch_order_sub(pdl_ctx *c, const OrderArgs &o, uint32_t wide_blocks) {
    const uint32_t rows_per_block = ORDER_THREADS / W, short_blocks = (o.n_rows + rows_per_block - 1) / rows_per_block;
    if (c->opt_order_wide_merged) { hipLaunchKernelGGL((k_order_rows_sub<W, true>), dim3(short_blocks + wide_blocks), dim3(ORDER_THREADS), 0, c->stream, o, short_blocks); return; }
    hipLaunchKernelGGL((k_order_rows_sub<W, false>), dim3(short_blocks), dim3(ORDER_THREADS), 0, c->stream, o, short_blocks);
    hipLaunchKernelGGL(k_order_rows, dim3(wide_blocks), dim3(ORDER_THREADS), 0, c->stream, o);
}
static void launch_order(pdl_ctx *c, const OrderArgs &o) {
    const uint32_t wide_blocks = std::min<uint32_t>(o.n_rows, (uint32_t) pdl_cus(c) * 8);
    const uint32_t w = order_sub_w(c);
    if (w == 16) return launch_order_sub<16>(c, o, wide_blocks);
    if (w == 32) return launch_order_sub<32>(c, o, wide_blocks);
    hipLaunchKernelGGL(k_order_rows_wave, dim3((o.n_rows + 3) / 4), dim3(256), 0, c->stream, o);
    hipLaunchKernelGGL(k_order_rows, dim3(wide_blocks), dim3(ORDER_THREADS), 0, c->stream, o);
}

static JoinArgs join_args(pdl_ctx *c, const ScorePlan &pl) {
    JoinArgs a{};
    a.post = pdl_postings(c); a.ranges = c->ranges.as<uint4>(); a.ranges8 = c->ranges8; a.seq_off = c->seq_off.as<uint32_t>();
    a.kseq_len = c->kseq_len.as<uint32_t>(); a.genome_of = c->d_gen; a.gene_info = c->gene_info.as<uint4>();
    a.task_lg = c->task_lg.as<uint32_t>();
    a.N = c->N; a.G = c->G; a.k = c->rp.k;
    a.min_kseq = (uint32_t) std::max<uint64_t>(c->min_kseq, 1); a.canonical = (c->flags & PDL_FLAG_CANONICAL_ORDER) ? 1u : 0u;
    a.MS = c->MS.as<float>(); a.CM = c->CM.as<float>();
    set_staged_cells(a, staged_cells(c)); a.st_cap = c->st_cap;
    a.mirror = pl.mirror ? 1u : 0u;
    a.sift_threshold = c->opt_sift_threshold ? 1u : 0u;
    if (pl.mirror) {
        a.taskpos_of = c->taskpos_of.as<uint32_t>(); a.local_genome = c->local_genome.as<uint32_t>();
        a.mirror_cnt = c->mirror_cnt.as<uint32_t>();
    }
    uint32_t *ctr32 = c->join_ctr.as<uint32_t>();
    a.error_count = ctr32 + PDL_JC_ERRORS; a.reload_count = ctr32 + PDL_JC_RELOADS;
    a.cell_cursor = reinterpret_cast<unsigned long long *>(ctr32 + PDL_JC_CELLS);
    return a;
}

// clears the maxima, the counters and the mirror bookkeeping (first_pass: the first pass since score_alloc_rows, whose
// descriptors ride in that launch with option "fused_glue"), then queues the tiers
static void score_join(pdl_ctx *c, const ScorePlan &pl, bool first_pass) {
    hipStream_t st = c->stream;
    const uint32_t N = c->N, G = c->G, n_rows = c->n_task_rows;
    const uint32_t S = (uint32_t) c->shard.size();
    {   // maxima, counters and (mirror mode) the per-row mirror counts/offsets/cursors start at zero: one launch
        auto n16 = [](size_t bytes) { return (unsigned long long) ((bytes + 15) / 16); };      // (buffers are sized in whole 16-byte words)
        ZeroRanges z{};
        z.p[0] = c->MS.as<uint4>(); z.n16[0] = n16((size_t) n_rows * G * sizeof(float));
        z.p[1] = c->CM.as<uint4>(); z.n16[1] = n16((size_t) S * N * sizeof(float));
        z.p[2] = c->join_ctr.as<uint4>(); z.n16[2] = n16(PDL_JC_WORDS * sizeof(uint32_t));
        z.p[3] = pl.mirror ? c->mirror_cnt.as<uint4>() : nullptr; z.n16[3] = pl.mirror ? n16((size_t) n_rows * 4 * 3) : 0;
        const unsigned long long most = std::max(z.n16[0], z.n16[1]);
        const uint32_t zero_blocks = (uint32_t) std::min<unsigned long long>((most + 255) / 256 + 1, (unsigned long long) c->cus * 16);
        if (first_pass && c->opt_fused_glue) {
            const uint32_t desc_blocks = row_desc_blocks(c);
            hipLaunchKernelGGL(k_open_pass, dim3(desc_blocks + zero_blocks), dim3(256), 0, st, row_desc_args(c), z, desc_blocks);
        } else hipLaunchKernelGGL(k_zero_ranges, dim3(zero_blocks), dim3(256), 0, st, z);
    }
    const JoinArgs a = join_args(c, pl);
    const JoinLists L{c->join_ctr.as<uint32_t>(), c->overflow_rows.as<uint32_t>(), c->row_desc2.as<uint4>(), c->row_desc.as<uint4>(), n_rows, pl.wide ? 0 : n_rows};

    ev_begin(c, EV_JOIN);
    if (pl.wide) {          // every row straight to tier 3: its link lists all task positions
        hipLaunchKernelGGL(k_iota_u32, dim3((n_rows + 255) / 256), dim3(256), 0, st, L.out(LINK_T2_T3).rows, n_rows);
        PDL_HIP(hipMemcpyAsync(L.out(LINK_T2_T3).count, &c->n_task_rows, 4, hipMemcpyHostToDevice, st));
    }
    // clear -> [tier 0 -> tier 0b] -> [tier 1] -> tier 2 -> tier 3: the first tier there is draws from every row, the others
    // from the link of the tier in front
    if (pl.tier0) {
        // the partition tier, and its second form (512 threads: twice the lookups per cycle) over the rows that alone exceed
        // the first form's cycle; what that cannot hold either is listed for tier 1
        launch_tier(c, a, pl.k0, pl.grid0, L.all(PDL_JC_CURSOR_T0, PT_BATCH), L.out(LINK_T0_T0B), &PHASES_T0);
        launch_tier(c, a, pl.k0b, pl.grid0b, L.in(LINK_T0_T0B), L.out(LINK_T0B_T1));
        c->tm.join_launches += 2;
    }
    if (pl.tier1) {
        JoinArgs a1 = a;
        if (pl.tier1 >= 9 && pl.tier1 <= 11) {
            // the filter tiers put a row's first sightings aside in a list per workgroup (16 bytes each; rewritten row after row, so
            // only the part in use is ever hot): room for 4x the lookups of the average row (never more than one per gene), a
            // row with more first sightings goes to tier 2
            const unsigned long long avg = n_rows ? c->P / n_rows : 0;
            a1.defer_cap = (uint32_t) std::min<unsigned long long>(std::min<unsigned long long>(std::max<unsigned long long>(4 * avg, 8192), 1u << 18), (unsigned long long) N + 64);
            a1.defer_wide = (N >= (1u << 22) || pl.wide_aside) ? 1u : 0u;
            c->join_defer.alloc((size_t) pl.grid1 * a1.defer_cap * (a1.defer_wide ? sizeof(uint4) : sizeof(uint2)));
            a1.defer = c->join_defer.p;
            static std::atomic<uint32_t> launch_serial{0};        // (process-wide: a freed list may come back to another context as it was left)
            a1.defer_serial = ++launch_serial;
        }
        launch_tier(c, a1, pl.k1, pl.grid1, pl.tier0 ? L.in(LINK_T0B_T1) : L.spread(PDL_JC_CURSOR_T1, pl.grid1), L.out(LINK_T1_T2), &PHASES_T1);
    }
    launch_tier(c, a, pl.k2, pl.grid2, pl.tier1 ? L.in(LINK_T1_T2) : L.spread(PDL_JC_CURSOR_T2, pl.grid2), L.out(LINK_T2_T3));
    PDL_HIP(hipGetLastError());
    // tier 3 (inside the join's event pair; its own pair is one of the optional stage timers)
    JoinArgs a3 = a; a3.hbm_acc = c->glb_table.as<unsigned long long>();
    a3.hbm_u32 = reinterpret_cast<uint32_t *>(c->glb_table.as<uint8_t>() + (size_t) pl.grid3 * hbm_layout(N, pl.wide).sums);
    ev_begin(c, EV_JOIN_OVF);
    c->glb_clean = false;
    launch_tier(c, a3, pl.k3, pl.grid3, L.in(LINK_T2_T3), TierOut{});
    PDL_HIP(hipGetLastError());
    ev_end(c, EV_JOIN_OVF);
    ev_end(c, EV_JOIN);
    c->tm.join_launches += 3;
}

// What the host reads of the join's counters after a pass, from the first words of join_ctr or of the gathered tail (PDL_JT_*:
// the same places).  A pass that broke an invariant of its own is an error.
struct JoinCounters {
    uint32_t rows_tier2, rows_tier3, reloads;
    unsigned long long cells;                // staging cells reserved (>= cells staged: chunk tails are unused)
};
static JoinCounters join_counters(const uint32_t *w, bool inbox_filed = false) {
    // (a multi-GPU pass has looked at the join's own count before the cells travelled: what is counted behind an inbox, the peers sent)
    if (w[PDL_JC_ERRORS] && inbox_filed)
        PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_dist_score_finish: %u received cells name a gene beyond the set or a column that is not a row of this rank; begin the pass again (pdl_dist_score_begin)", w[PDL_JC_ERRORS]);
    if (w[PDL_JC_ERRORS]) PDL_FAIL(PDL_ERR_DEVICE, "join: %u internal consistency violations", w[PDL_JC_ERRORS]);
    JoinCounters j{w[PDL_JC_ROWS_T2], w[PDL_JC_ROWS_T3], w[PDL_JC_RELOADS], 0};
    memcpy(&j.cells, w + PDL_JC_CELLS, sizeof(j.cells));
    return j;
}

// K-order over the staged cells (+ the n_inbox cells filed at slots st_cap ..), then the one look at the counters.
// Returns the staging cells the join asked for (> st_cap: the pass must be repeated).
static unsigned long long score_order(pdl_ctx *c, const ScorePlan &pl, const pdl_dist_cell *d_inbox, uint32_t n_inbox, int ev_total) {
    hipStream_t st = c->stream;
    const uint32_t n_rows = c->n_task_rows;
    const uint32_t S = (uint32_t) c->shard.size();
    uint64_t *d_scal = c->scalars.as<uint64_t>();
    uint32_t *ctr32 = c->join_ctr.as<uint32_t>();
    ev_begin(c, EV_ORDER);
    const uint32_t *d_mcnt = pl.mirror ? c->mirror_cnt.as<uint32_t>() : nullptr;
    // mirror mode, a row count within the bound: both offset arrays and both totals from k_order_offsets; else the scans
    const bool one_launch = pl.mirror && c->opt_order_offsets != 0 && n_rows > 0 && n_rows <= std::min(c->opt_order_offsets_rows, OO_MAX_ROWS);
    if (one_launch) {
        const uint32_t span = c->opt_order_offsets == 1 ? (n_rows + OO_TILE - 1) / OO_TILE * OO_TILE : OO_TILE;        // one workgroup, or one per OO_TILE rows
        hipLaunchKernelGGL(k_order_offsets, dim3((n_rows + span - 1) / span), dim3(OO_THREADS), 0, st, c->row_cnt.as<uint32_t>(), d_mcnt, n_rows, span,
                           c->fin_off.as<uint32_t>(), c->mirror_cnt.as<uint32_t>() + n_rows, d_scal + PDL_CTL_EMITTED, d_scal + PDL_CTL_MIRRORED);
    } else {
        // the scan's total (all emitted cells, < 2^32) also closes fin_off: the low word of the u64 lands in fin_off[n_rows]
        scan_and_apply(c, n_rows, RowCntFlag{c->row_cnt.as<uint32_t>(), d_mcnt}, FinOffApply{c->fin_off.as<uint32_t>()}, d_scal + PDL_CTL_EMITTED,
                       reinterpret_cast<uint64_t *>(c->fin_off.as<uint32_t>() + n_rows));
    }
    OrderArgs o{};
    if (pl.mirror) {
        uint32_t *m_off = c->mirror_cnt.as<uint32_t>() + n_rows, *m_cur = m_off + n_rows;
        if (!one_launch) scan_and_apply(c, n_rows, MirrorCntFlag{d_mcnt}, FinOffApply{m_off}, d_scal + PDL_CTL_MIRRORED);
        MirrorArgs ma{};
        set_staged_cells(ma, staged_cells(c));
        ma.taskpos_of = c->taskpos_of.as<uint32_t>(); ma.mirror_off = m_off; ma.mirror_cur = m_cur; ma.n_rows = n_rows;
        ma.mcell = c->mirror_ref.as<MCell>();
        const uint32_t w = order_sub_w(c);
        if (w == 16) hipLaunchKernelGGL(k_mirror_cells_sub<16>, dim3((n_rows + 15) / 16), dim3(256), 0, st, ma);
        else if (w == 32) hipLaunchKernelGGL(k_mirror_cells_sub<32>, dim3((n_rows + 7) / 8), dim3(256), 0, st, ma);
        else hipLaunchKernelGGL(k_mirror_cells, dim3((n_rows + 3) / 4), dim3(256), 0, st, ma);
        if (n_inbox) hipLaunchKernelGGL(k_mirror_cells_inbox, dim3((n_inbox + 255) / 256), dim3(256), 0, st, ma, d_inbox, n_inbox, c->N);
        o.mirror_cnt = d_mcnt; o.mirror_off = m_off; o.mcell = c->mirror_ref.as<MCell>();
    }
    set_staged_cells(o, staged_cells(c)); o.fin_off = c->fin_off.as<uint32_t>();
    o.c_score = c->c_score.as<float>(); o.c_perc = c->c_perc.as<float>(); o.c_tr = c->c_tr.as<float>();
    o.c_row = c->c_row.as<int32_t>(); o.c_col = c->c_col.as<int32_t>();
    o.n_rows = n_rows; o.canonical = (c->flags & PDL_FLAG_CANONICAL_ORDER) ? 1u : 0u; o.pack_ok = c->N < (1u << 22) ? 1u : 0u;
    o.wide_rows = ctr32 + PDL_JC_WIDE_ROWS;  // (counter block, zero since the clearing launch)
    launch_order(c, o);
    PDL_HIP(hipGetLastError());
    ev_end(c, EV_ORDER);

    // first cell of every shard genome = fin_off at its first task row; then the one look at the counters
    uint32_t *d_idx = c->task_off.as<uint32_t>();
    uint32_t *d_out = d_idx + (S + 1);
    hipLaunchKernelGGL(k_gather_u32, dim3((S + 1 + PDL_JT_WORDS + 255) / 256), dim3(256), 0, st, c->fin_off.as<uint32_t>(), d_idx, S + 1, d_out,
                       ctr32, reinterpret_cast<const uint32_t *>(d_scal + PDL_CTL_EMITTED));
    c->h_fin.resize(S + 1);
    JoinCounters jc;
    uint64_t zsum = 0;
    {
        PinRead rd(c);
        const uint32_t *pf = rd.add<uint32_t>(d_out, S + 1 + PDL_JT_WORDS);
        const uint32_t *lbe = lookback_error_word(c, rd);
        ev_end(c, ev_total);
        rd.sync();
        lookback_check(c, lbe);
        memcpy(c->h_fin.data(), pf, (size_t) (S + 1) * 4);
        const uint32_t *tail = pf + S + 1;
        memcpy(&zsum, tail + PDL_JT_EMITTED, sizeof(zsum));
        c->tm.tier1_rows = pl.tier0 ? tail[PDL_JT_ROWS_T1] : (pl.tier1 ? n_rows : 0);
        c->glb_clean = true;
        jc = join_counters(tail, n_inbox != 0);
    }
    c->tm.aside_reloads = jc.reloads;
    c->tm.overflow_rows = jc.rows_tier3;
    c->tm.tier2_rows = pl.tier1 ? jc.rows_tier2 : n_rows;
    if (jc.cells <= c->st_cap) {
        c->Z = zsum;
        c->tm.emitted_cells = c->Z;
        for (uint32_t i = 0; i <= S; i++) c->h_cell_off[i] = c->h_fin[i];
    }
    return jc.cells;
}

// after a join: did a pass with 10-bit tagged put-aside entries see one that had to be loaded again (or does the test switch say so)?
static bool aside_pass_is_suspect(pdl_ctx *c, const ScorePlan &pl) {
    if (pl.wide_aside || c->N >= (1u << 22) || pl.wide || !(pl.tier1 >= 9 && pl.tier1 <= 11)) return false;      // fully tagged entries, or no list at all
    const bool seen = c->tm.aside_reloads != 0 || c->opt_aside_test_reload;
    c->opt_aside_test_reload = false;
    return seen;
}

// The verdict on a pass, given the staging cells `z` it asked for; a repeat is prepared here (wide entries / the cap asked for).
// The canary acts: a pass whose 8-byte put-aside entries (10-bit tag) needed a second look is not trusted — a stale
// entry passes that tag once in 1024 — and is repeated with entries that name row and launch in full, where a reload
// is exact.  (Never seen outside the test switch: the cost falls on a path that does not fire.)
enum class PassVerdict { accept, repeat_wide_aside, repeat_with_cap };
static PassVerdict judge_pass(pdl_ctx *c, ScorePlan &pl, unsigned long long z, unsigned long long &cap, int attempt, int &overflows) {
    if (aside_pass_is_suspect(c, pl)) {
        if (attempt > 3) PDL_FAIL(PDL_ERR_DEVICE, "put-aside list: reloads persisted");
        pl.wide_aside = true; c->tm.aside_repeats++;
        return PassVerdict::repeat_wide_aside;
    }
    if (z <= cap) return PassVerdict::accept;
    if (++overflows == 2) PDL_FAIL(PDL_ERR_DEVICE, "staging overflow persisted (%llu cells > %llu)", z, cap);
    cap = z + pl.slack;          // what was asked for plus chunk slack, second and last attempt
    return PassVerdict::repeat_with_cap;
}

static unsigned long long first_staging_cap(pdl_ctx *c, const ScorePlan &pl, uint64_t lookups) {
    // staging capacity: emitted cells are, in practice, the homologous pairs (about one per genome and row);
    // if the guess is short the pass is repeated once with the exact size ("staging_cap" forces that in tests)
    if (c->opt_staging_cap) return c->opt_staging_cap;
    unsigned long long cap = std::max<unsigned long long>(1ull << 20, (unsigned long long) c->n_task_rows * (c->G + 16ull));
    return std::min<unsigned long long>(cap, std::max<unsigned long long>(lookups, 1ull)) + pl.slack;
}

static void join_timings(pdl_ctx *c) { c->tm.join_ms = ev_ms(c, EV_JOIN); c->tm.join_overflow_ms = ev_ms(c, EV_JOIN_OVF); }

static void score_reset(pdl_ctx *c) {
    const uint32_t S = (uint32_t) c->shard.size();
    c->h_cell_off.assign(S + 1, 0);
    c->Z = 0;
    c->tm.emitted_cells = 0; c->tm.scored_rows = c->n_task_rows; c->tm.overflow_rows = 0; c->tm.join_launches = 0; c->tm.aside_repeats = 0; c->tm.aside_reloads = 0;
    c->tm.scored_lookups = 0; c->tm.walked_lookups = 0; c->tm.outbox_cells = c->tm.inbox_cells = 0;
    c->tm.dist_score_begin_ms = c->tm.dist_score_finish_ms = 0.f;
    if (c->costs_ready) for (uint32_t i = 0; i < S; i++) c->tm.scored_lookups += c->h_genome_cost[c->shard[i]];
    else c->tm.scored_lookups = c->P;         // (packed ranges: the total of this context's genomes, per-genome values on demand)
}

void pdl_run_score_all(pdl_ctx *c) {
    ev_begin(c, EV_SCORE_TOTAL);
    if (!c->tasks_ready) pdl_prepare_tasks(c);
    score_reset(c);
    if (c->n_task_rows == 0) { c->scored = true; ev_end(c, EV_SCORE_TOTAL); return; }
    ScorePlan pl = score_plan(c);
    c->tm.walked_lookups = pl.mirror ? (c->P - c->Ushared) / 2 : c->tm.scored_lookups;       // sum s(s-1)/2 = (sum s^2 - sum s) / 2
    score_alloc_rows(c, pl);
    unsigned long long cap = first_staging_cap(c, pl, c->P);
    for (int attempt = 0, overflows = 0;; attempt++) {
        score_alloc_cells(c, pl, cap, 0);
        score_join(c, pl, attempt == 0);
        const unsigned long long z = score_order(c, pl, nullptr, 0, EV_SCORE_TOTAL);
        if (judge_pass(c, pl, z, cap, attempt, overflows) == PassVerdict::accept) break;
        ev_begin(c, EV_SCORE_TOTAL);
    }
    join_timings(c);
    c->tm.order_ms = ev_ms(c, EV_ORDER);
    c->tm.score_total_ms = ev_ms(c, EV_SCORE_TOTAL);
    c->scored = true;
}

// ---- multi-GPU scoring ------------------------------------------------------------------------------------------
void pdl_run_dist_score_begin(pdl_ctx *c) {
    hipStream_t st = c->stream;
    ev_begin(c, EV_SCORE_TOTAL);
    if (!c->tasks_ready) pdl_prepare_tasks(c);
    score_reset(c);
    const uint32_t W = c->world, n_rows = c->n_task_rows;
    if (W > PDL_MAX_WORLD) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than %u ranks", PDL_MAX_WORLD);
    c->h_outbox_counts.assign(W, 0);
    c->st_local = 0; c->n_inbox = 0;
    uint64_t upper = 0;
    for (uint32_t g : c->shard) upper += c->h_upper_cost[g];
    c->tm.walked_lookups = upper;
    if (n_rows == 0) { ev_end(c, EV_SCORE_TOTAL); PDL_HIP(hipStreamSynchronize(st)); c->dist_stage = DistStage::joined; return; }
    ScorePlan pl = score_plan(c);
    if (!pl.mirror) PDL_FAIL(PDL_ERR_STATE, "multi-GPU scoring needs the upper-triangle range lists of pdl_dist_preprocess_finish");
    score_alloc_rows(c, pl);
    uint64_t *d_outbox_total = c->scalars.as<uint64_t>() + PDL_CTL_OUTBOX_TOTAL;
    // outbox listing: rows are dealt to workgroups in blocks
    const uint32_t n_blocks = std::max<uint32_t>(1, std::min<uint32_t>((n_rows + 15) / 16, 2048));
    const uint32_t rows_per_block = (n_rows + n_blocks - 1) / n_blocks;
    const size_t tab_n = (size_t) W * n_blocks;
    c->outbox_tab.alloc((2 * tab_n + W + 2) * sizeof(uint32_t));
    uint32_t *tab = c->outbox_tab.as<uint32_t>(), *offs = tab + tab_n, *d_tot = offs + tab_n;
    unsigned long long cap = first_staging_cap(c, pl, std::max<uint64_t>(upper, 1));
    for (int attempt = 0, overflows = 0;; attempt++) {
        // room for as many received cells as staged ones right away (the exchange is symmetric on average); grown if short
        score_alloc_cells(c, pl, cap, cap);
        score_join(c, pl, attempt == 0);
        OutboxArgs oa{};
        set_staged_cells(oa, staged_cells(c));
        oa.taskpos_of = c->taskpos_of.as<uint32_t>(); oa.genome_of = c->d_gen; oa.owner = c->owner_of_genome.as<uint32_t>();
        oa.n_rows = n_rows; oa.rows_per_block = rows_per_block; oa.world = W; oa.n_blocks = n_blocks;
        oa.tab = tab; oa.offs = offs;
        hipLaunchKernelGGL(k_outbox<false>, dim3(n_blocks), dim3(256), 0, st, oa);
        scan_and_apply(c, tab_n, RowCntFlag{tab, nullptr}, FinOffApply{offs}, d_outbox_total);
        hipLaunchKernelGGL(k_outbox_totals, dim3(1), dim3(PDL_MAX_WORLD + 1 < 128 ? 128 : PDL_MAX_WORLD + 1), 0, st, offs, n_blocks, W, d_outbox_total, d_tot);
        PDL_HIP(hipGetLastError());
        uint32_t h_tot[PDL_MAX_WORLD + 1];
        JoinCounters jc;
        {
            PinRead rd(c);
            const uint32_t *pt = rd.add<uint32_t>(d_tot, W + 1);
            const uint32_t *pc = rd.add<uint32_t>(c->join_ctr.as<uint32_t>(), PDL_JC_RELOADS + 1);
            rd.sync();
            memcpy(h_tot, pt, (W + 1) * 4);
            c->glb_clean = true;             // (k_join_hbm has run to its end and left its tables zeroed)
            jc = join_counters(pc);
        }
        c->tm.aside_reloads = jc.reloads;
        if (judge_pass(c, pl, jc.cells, cap, attempt, overflows) != PassVerdict::accept) continue;
        const uint64_t total = h_tot[W];
        for (uint32_t d = 0; d < W; d++) c->h_outbox_counts[d] = (d + 1 < W ? h_tot[d + 1] : total) - h_tot[d];
        c->outbox.alloc(std::max<uint64_t>(total, 1) * sizeof(pdl_dist_cell));
        if (total) {
            oa.out = c->outbox.as<pdl_dist_cell>();
            hipLaunchKernelGGL(k_outbox<true>, dim3(n_blocks), dim3(256), 0, st, oa);
            PDL_HIP(hipGetLastError());
        }
        c->tm.outbox_cells = total;
        break;
    }
    ev_end(c, EV_SCORE_TOTAL);
    PDL_HIP(hipStreamSynchronize(st));
    join_timings(c);
    c->tm.dist_score_begin_ms = ev_ms(c, EV_SCORE_TOTAL);
    c->dist_stage = DistStage::joined;
}

void pdl_run_dist_score_finish(pdl_ctx *c, const pdl_dist_cell *d_inbox, uint64_t n_inbox) {
    hipStream_t st = c->stream;
    ev_begin(c, EV_DIST_SCORE_FINISH);
    const uint32_t n_rows = c->n_task_rows;
    c->tm.inbox_cells = n_inbox;
    if (n_rows == 0) {
        if (n_inbox) PDL_FAIL(PDL_ERR_ARGUMENT, "pdl_dist_score_finish: %llu cells received by a rank without rows", (unsigned long long) n_inbox);
        ev_end(c, EV_DIST_SCORE_FINISH); c->scored = true; c->dist_stage = DistStage::scored; return;
    }
    // (from here on the call counts cells into the rows and folds them into the maxima: one that fails leaves the pass to be begun again)
    c->dist_stage = DistStage::adopted;
    const ScorePlan pl = score_plan(c);
    const unsigned long long cap = c->st_cap;
    if (n_inbox > cap) score_alloc_cells(c, pl, cap, n_inbox);             // (rare: the first allocation leaves room for `cap` received cells)
    else if (2 * cap + n_inbox >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 emitted cells on one device");
    if (n_inbox) {
        InboxArgs ia{};
        ia.in = d_inbox; ia.n = (uint32_t) n_inbox;
        ia.taskpos_of = c->taskpos_of.as<uint32_t>(); ia.genome_of = c->d_gen; ia.local_genome = c->local_genome.as<uint32_t>();
        ia.mirror_cnt = c->mirror_cnt.as<uint32_t>(); ia.MS = c->MS.as<float>(); ia.CM = c->CM.as<float>();
        ia.N = c->N; ia.G = c->G; ia.error_count = c->join_ctr.as<uint32_t>() + PDL_JC_ERRORS;
        hipLaunchKernelGGL(k_inbox_file, dim3((uint32_t) ((n_inbox + 255) / 256)), dim3(256), 0, st, ia);
        PDL_HIP(hipGetLastError());
    }
    const unsigned long long z = score_order(c, pl, d_inbox, (uint32_t) n_inbox, EV_DIST_SCORE_FINISH);
    if (z > cap) PDL_FAIL(PDL_ERR_DEVICE, "staging cursor moved after the join (%llu > %llu)", z, cap);
    c->tm.order_ms = ev_ms(c, EV_ORDER);
    c->tm.dist_score_finish_ms = ev_ms(c, EV_DIST_SCORE_FINISH);
    c->tm.score_total_ms = c->tm.dist_score_begin_ms + c->tm.dist_score_finish_ms;
    c->scored = true;
    c->dist_stage = DistStage::scored;
}

#include "pdl_query.h"           // K-query: one new genome against this dictionary (pdl_query_scores)
#include "pdl_query_batch.h"     // ... and a batch of them, each on its own (pdl_query_batch)
