// pdl_query_batch.h — K-query for a batch: q new genomes scored against the dictionary that is already in HBM, each on its own
// (pdl_query_batch, include/pandelos_amd.h), included from pdl_join.hip behind pdl_query.h, whose group description (QDesc),
// row walk, finalize and HBM table layout it reuses.  The single query's kernels and host path are not touched.
//
// Contract: block j is what pdl_query_scores returns for genome j alone — computeScores(G) of base + genome j.  The queries
// never see each other; the base context is only read.
//
// One genome cannot fill the chip (the match is one round of latency, the join has fewer workgroups than the chip
// holds, the launches and host reads are a third of the time), so the stages run ONCE over all genes of a chunk of queries:
//
//   B-alpha  k_qb_alpha     every query byte against the base's letters; per query the smallest absent byte
//   B-dict   pdl_query_dictionary over all genes of the chunk (gene value = position in the chunk): records in (rank, gene) order
//   B-seg    k_qb_seg_key + pdl_sort_pairs (stable, key = query) + k_qb_gather: every query's records as ONE segment in
//            (rank, gene) order — rank and {gene local to the query, count} copied out, so a probe is one load
//   B-fold   k_qb_fold      one thread per query: the base's fold and the union's (pdl_query.h, Q1), cases (a)-(d) per query
//   B-match  k_qb_match     one thread per record of the chunk: base searches as the single query's, query searches inside the
//                           record's own segment; cost, matched count per query
//   B-rows   gene sort of the records (pdl_sort_pairs) + k_qb_row_off: each gene's records in rank order; staging bound per query
//   B-join   k_qb_join      one workgroup per gene of the chunk: the single query's row program with the fold-free arguments of
//            k_qb_join_hbm  the gene's query (its slices of the maxima); rows that leave the LDS table: HBM tables laid out for
//                           N + (largest query of the batch) columns
//   B-order  k_order_rows_wave / k_order_rows once over the chunk's rows; k_qb_counts: cells per query
//
// Positions of query records (QDesc.qlo/qhi/qextra, QFold.qL) are positions in the segmented arrays of the chunk; QDesc.key is
// taken relative to the segment start, so it is the single query's key.
#pragma once
#include "pdl_query.h"

// control words of a chunk (qbb.ctl, u64): QBG_WORDS for the chunk, then QB_CTL_WORDS per query; cleared at the start of every
// chunk, each word has one life
enum : uint32_t {
    QBG_RECORDS = 0,            // records of the chunk's dictionary (total of its dedup scan)
    QBG_OVERFLOW_ROWS = 1,      // rows the LDS join handed to the HBM join
    QBG_CELL_CURSOR = 2,        // staging cursor
    QBG_EMITTED = 3,            // emitted cells (total of the row-count scan)
    QBG_WIDE_ROWS = 4,          // order: rows of more than 256 cells
    QBG_WORDS = 8,
};
enum : uint32_t {
    QB_CTL_RECORDS = 0,         // records of the query (its segment)
    QB_CTL_BAD_BYTE = 1,        // 256 - smallest byte that is not in the base's alphabet (0: none)
    QB_CTL_COST = 2,            // genome cost
    QB_CTL_MATCHED = 3,         // matched records
    QB_CTL_BOUND = 4,           // staging bound
    QB_CTL_MAY_OVERFLOW = 5,    // rows that may overflow (more lookups than the LDS table holds keys)
    QB_CTL_EMITTED = 6,         // emitted cells
    QB_CTL_WORDS = 8,
};
__device__ __forceinline__ unsigned long long *qb_ctl(unsigned long long *ctl, uint32_t q) { return ctl + QBG_WORDS + (size_t) q * QB_CTL_WORDS; }

// the chunk's layout: genes [gene_begin[q], gene_begin[q + 1]) and bytes [res_begin[q], res_begin[q + 1]) belong to query q
struct QBLayout {
    const uint32_t *gene_begin;     // [nq + 1]
    const uint64_t *res_begin;      // [nq + 1]
    const uint32_t *gene_query;     // [genes]
    uint32_t nq, genes;
};

struct QBAlphaArgs { const uint8_t *res; uint64_t n; uint32_t present[8]; QBLayout lay; unsigned long long *ctl; };
__global__ __launch_bounds__(256) void k_qb_alpha(QBAlphaArgs a) {
    for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < a.n; i += (uint64_t) gridDim.x * 256) {
        const uint32_t b = a.res[i];
        if ((a.present[b >> 5] >> (b & 31)) & 1u) continue;
        uint32_t lo = 0, hi = a.lay.nq;                       // last query q with res_begin[q] <= i (absent bytes are rare: searched only then)
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (a.lay.res_begin[m] <= i) lo = m; else hi = m; }
        atomicMax(qb_ctl(a.ctl, lo) + QB_CTL_BAD_BYTE, (unsigned long long) (256u - b));
    }
}

// key of the segment sort: the query of every record of the chunk's dictionary
__global__ __launch_bounds__(256) void k_qb_seg_key(const uint2 *post, const unsigned long long *ctl, QBLayout lay, uint32_t *key) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u < (uint32_t) ctl[QBG_RECORDS]) key[u] = lay.gene_query[post[u].x];
}

// Records in segment order: rank and {local gene, count} of position j, and seg_off[q] = first position of query q (a query
// without records gets an empty segment; seg_off was cleared, which is right for a chunk without records).
template <class KeyT>
__global__ __launch_bounds__(256) void k_qb_gather(const KeyT *keys, const uint32_t *recpos, const uint2 *post, const uint32_t *perm,
                                                   const uint32_t *qid_sorted, const unsigned long long *ctl, QBLayout lay,
                                                   KeyT *srank, uint2 *spost, uint32_t *seg_off) {
    const uint32_t U = (uint32_t) ctl[QBG_RECORDS];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= U) return;
    const uint32_t src = perm[j], q = qid_sorted[j];
    srank[j] = keys[recpos[src]];
    const uint2 p = post[src];
    spost[j] = make_uint2(p.x - lay.gene_begin[q], p.y);
    const uint32_t prev = j ? qid_sorted[j - 1] : Q_NONE;     // (Q_NONE + 1 == 0)
    for (uint32_t s = prev + 1; s <= q; s++) seg_off[s] = j;
    if (j == U - 1) for (uint32_t s = q + 1; s <= lay.nq; s++) seg_off[s] = U;
}

template <class KeyT> struct QBView {
    QView<KeyT> b;                  // the base half (bkeys, brecpos, bvals, post, U, M); its query half is not used
    const KeyT *srank; const uint2 *spost;
    const uint32_t *seg_off, *qid_sorted;
    __device__ unsigned long long qrank(uint32_t j) const { return (unsigned long long) srank[j]; }
    template <bool UPPER> __device__ uint32_t qbound(uint32_t lo, uint32_t hi, unsigned long long v) const {
        while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); const unsigned long long r = qrank(m); if (UPPER ? r <= v : r < v) lo = m + 1; else hi = m; }
        return lo;
    }
};

// One thread per query: the base's fold (the same for all, computed by each) and the union's with this query's largest rank.
template <class KeyT>
__global__ __launch_bounds__(64) void k_qb_fold(QBView<KeyT> v, uint32_t nq, unsigned long long *ctl, QFold *out) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    QFold f{};
    f.p = Q_NONE; f.qL = Q_NONE;
    const uint32_t s0 = v.seg_off[q], s1 = v.seg_off[q + 1], Uq = s1 - s0;
    qb_ctl(ctl, q)[QB_CTL_RECORDS] = Uq;
    if (Uq == 0) { out[q] = f; return; }                          // no k-mer: no record reads the fold
    const uint32_t U = v.b.U;
    f.bmax = (unsigned long long) v.b.bkeys[v.b.M - 1];
    bool lonely = U == 1;
    bool has_r2 = false;
    if (U == 1) f.p = 0;
    else {
        const unsigned long long rl = v.b.brank(U - 1), rl2 = v.b.brank(U - 2);
        f.folded = (rl != f.bmax || rl2 != f.bmax) ? 1u : 0u;
        if (f.folded) {
            lonely = has_r2 = true;
            f.r2 = rl != f.bmax ? rl : rl2;
            f.gs = v.b.template bbound<false>(0, U, f.r2);
            const uint32_t gl = v.b.bvals[v.b.M - 1];
            uint32_t lo = f.gs, hi = U;
            while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (v.b.post[m].x < gl) lo = m + 1; else hi = m; }
            if (v.b.brank(lo) != f.bmax) lo++;
            f.p = lo;
        }
    }
    const unsigned long long qmax = v.qrank(s1 - 1);
    const bool alone = Uq == 1 || v.qrank(s1 - 2) != qmax;
    if (qmax > f.bmax) {
        f.skip_p = f.folded;
        if (alone) {
            f.qL = s1 - 1;
            const unsigned long long q2 = Uq >= 2 ? v.qrank(s1 - 2) : 0ull;
            f.tgt = (Uq >= 2 && q2 > f.bmax) ? q2 : f.bmax;
        }
    } else if (qmax == f.bmax) {
        f.skip_p = f.folded;
    } else if (lonely && (!has_r2 || qmax > f.r2)) {
        f.skip_p = f.folded; f.has_extra = 1; f.extra_target = qmax;
    }
    out[q] = f;
}

struct QBMatchOut {
    QDesc *desc; uint32_t *gene_key; uint32_t *row_lookups;
    unsigned long long *ctl;
};
template <class KeyT>
__global__ __launch_bounds__(256) void k_qb_match(QBView<KeyT> v, const QFold *folds, QBLayout lay, QBMatchOut o, uint64_t bound) {
    const uint32_t Ut = (uint32_t) o.ctl[QBG_RECORDS];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    unsigned long long cost = 0, matched = 0;
    uint32_t q = Q_NONE;
    if (j < Ut && j < bound) {
        q = v.qid_sorted[j];
        const QFold f = folds[q];
        const uint32_t s0 = v.seg_off[q], s1 = v.seg_off[q + 1];
        const unsigned long long r = v.qrank(j);
        const unsigned long long eff = j == f.qL ? f.tgt : r;
        QDesc d;
        d.blo = d.bhi = 0; d.bskip = d.bextra = d.qextra = Q_NONE;
        if (f.folded) {
            if (eff < f.r2) { d.blo = v.b.template bbound<false>(0, f.gs, eff); d.bhi = v.b.template bbound<true>(d.blo, f.gs, eff); }
            else if (eff == f.r2) { d.blo = f.gs; d.bhi = v.b.U; if (f.skip_p) d.bskip = f.p; }
            else if (eff == f.bmax) { d.blo = f.p; d.bhi = f.p + 1; }
        } else {
            d.blo = v.b.template bbound<false>(0, v.b.U, eff); d.bhi = v.b.template bbound<true>(d.blo, v.b.U, eff);
        }
        if (f.has_extra && eff == f.extra_target) d.bextra = f.p;
        const uint32_t qn = f.qL != Q_NONE ? s1 - 1 : s1;         // searches among query records stay inside the record's own segment
        d.qlo = v.template qbound<false>(s0, qn, eff); d.qhi = v.template qbound<true>(d.qlo, qn, eff);
        if (f.qL != Q_NONE && eff == f.tgt) d.qextra = f.qL;
        d.key = 2u * (d.qlo - s0) + (d.qhi > d.qlo ? 1u : 0u);
        const uint32_t sz = q_size(d);
        o.desc[j] = d;
        const uint32_t gene = lay.gene_begin[q] + v.spost[j].x;
        o.gene_key[j] = gene;
        if (sz >= 2) { cost = sz; atomicAdd(&o.row_lookups[gene], sz); }
        matched = (j != f.qL && d.bhi > d.blo) ? 1ull : 0ull;
    }
    // a wave inside one segment (nearly all of them) adds up by shuffles; one that straddles queries lets every lane add its own
    const uint32_t q0 = (uint32_t) __shfl((int) q, 0, PDL_WAVE);
    if (__all(q == q0)) {
        if (q0 == Q_NONE) return;
#pragma unroll
        for (int s = PDL_WAVE / 2; s > 0; s >>= 1) { cost += __shfl_down(cost, s, PDL_WAVE); matched += __shfl_down(matched, s, PDL_WAVE); }
        if ((threadIdx.x & (PDL_WAVE - 1)) != 0) return;
    }
    if (q == Q_NONE) return;
    if (cost) atomicAdd(qb_ctl(o.ctl, q) + QB_CTL_COST, cost);
    if (matched) atomicAdd(qb_ctl(o.ctl, q) + QB_CTL_MATCHED, matched);
}

// row_off[g] = first position of chunk gene g in the gene-sorted records; per query: staging bound = sum of
// min(lookups, columns of ITS union), rows whose lookups exceed `limit`; rowid[g] = the gene's id in its union
__global__ __launch_bounds__(256) void k_qb_row_off(const uint32_t *gene_sorted, unsigned long long *ctl, QBLayout lay, uint32_t N, uint32_t *row_off,
                                                    const uint32_t *row_lookups, uint32_t limit, uint32_t *rowid) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t Ut = (uint32_t) ctl[QBG_RECORDS];
    if (g > lay.genes) return;
    uint32_t lo = 0, hi = Ut;
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (gene_sorted[m] < g) lo = m + 1; else hi = m; }
    row_off[g] = lo;
    if (g == lay.genes) return;
    const uint32_t q = lay.gene_query[g], g0 = lay.gene_begin[q];
    rowid[g] = N + (g - g0);
    const uint32_t n_cols = N + (lay.gene_begin[q + 1] - g0), l = row_lookups[g];
    if (l) atomicAdd(qb_ctl(ctl, q) + QB_CTL_BOUND, (unsigned long long) min(l, n_cols));
    if (l > limit) atomicAdd(qb_ctl(ctl, q) + QB_CTL_MAY_OVERFLOW, 1ull);
}

// ---- B-join ------------------------------------------------------------------------------------------------------------
// `a` holds the chunk-wide arrays (rows, maxima and k-mer counts indexed by chunk gene; CM: the queries' [N + n_q] slices one
// behind the other); qb_row_args cuts out what the single query's row program sees for chunk gene gg: its query's slices.
struct QBJoinArgs {
    QJoinArgs a;
    QBLayout lay;
    uint32_t hbm_cols;              // columns the HBM tables are laid out for: N + the largest query of the batch
};
__device__ __forceinline__ QJoinArgs qb_row_args(const QBJoinArgs &b, uint32_t gg, uint32_t &g) {
    QJoinArgs a = b.a;
    const uint32_t q = b.lay.gene_query[gg], g0 = b.lay.gene_begin[q];
    g = gg - g0;
    a.n = b.lay.gene_begin[q + 1] - g0;
    a.row_off += g0; a.kseq_q += g0; a.row_base += g0; a.row_cnt += g0;
    a.MS += (size_t) g0 * a.G1;
    a.CM += (size_t) q * a.N + g0;
    return a;
}

__global__ __launch_bounds__(QJ_T) void k_qb_join(QBJoinArgs b) {
    __shared__ uint32_t s_key[QJ_HT], s_first[QJ_HT];
    __shared__ unsigned long long s_acc[QJ_HT];
    __shared__ QDesc s_d[QJ_T];
    __shared__ uint32_t s_cnt[QJ_T], s_pre[QJ_T + 1 + QJ_T / PDL_WAVE];
    __shared__ uint32_t s_nkeys, s_stop, s_ncell;
    __shared__ unsigned long long s_cbase;
    uint32_t g;
    const QJoinArgs a = qb_row_args(b, blockIdx.x, g);
    if (a.row_off[g] == a.row_off[g + 1]) {               // (uniform) no k-mer, no cell
        if (threadIdx.x == 0) { a.row_cnt[g] = 0; a.row_base[g] = 0; }
        return;
    }
    for (uint32_t i = threadIdx.x; i < QJ_HT; i += QJ_T) { s_key[i] = EMPTY_KEY; s_first[i] = 0xffffffffu; s_acc[i] = 0; }
    if (threadIdx.x == 0) { s_nkeys = 0; s_stop = 0; s_ncell = 0; }
    pdl_sync();
    q_walk_row(a, g, s_d, s_cnt, s_pre, &s_stop, [&](uint32_t col, unsigned long long packed, uint32_t key) -> bool {
        uint32_t h = (col * 2654435761u) >> (32 - QJ_HT_BITS);
        for (;;) {
            const uint32_t k = *(volatile uint32_t *) &s_key[h];
            if (k == col) break;
            if (k == EMPTY_KEY) {
                if (*(volatile uint32_t *) &s_nkeys >= QJ_LIMIT) return false;
                const uint32_t old = atomicCAS(&s_key[h], EMPTY_KEY, col);
                if (old == EMPTY_KEY) { atomicAdd(&s_nkeys, 1u); break; }
                if (old == col) break;
            }
            h = (h + 1) & (QJ_HT - 1);
        }
        atomicAdd(&s_acc[h], packed);
        atomicMin(&s_first[h], key);
        return true;
    });
    if (s_stop) {                                         // (uniform: read after the walk's last barrier) more columns than the table holds
        if (threadIdx.x == 0) {
            const unsigned long long i = atomicAdd(a.n_overflow, 1ull);
            a.overflow_rows[i] = blockIdx.x;              // (the chunk gene: k_qb_join_hbm cuts its query's slices out again)
            a.row_cnt[g] = 0; a.row_base[g] = 0;
        }
        return;
    }
    float sc[QJ_SLOTS], pc[QJ_SLOTS], tc[QJ_SLOTS];
    uint32_t at[QJ_SLOTS];
#pragma unroll
    for (uint32_t s = 0; s < QJ_SLOTS; s++) {
        const uint32_t i = s * QJ_T + threadIdx.x;
        at[s] = Q_NONE; sc[s] = 0.f; pc[s] = 0.f; tc[s] = 0.f;
        const uint32_t col = s_key[i];
        if (col != EMPTY_KEY) {
            sc[s] = q_finalize(a, g, col, s_acc[i], pc[s], tc[s]);
            if (sc[s] > 0.0f) at[s] = atomicAdd(&s_ncell, 1u);
        }
    }
    pdl_sync();
    if (threadIdx.x == 0) {
        s_cbase = atomicAdd(a.cell_cursor, (unsigned long long) s_ncell);
        a.row_base[g] = (uint32_t) s_cbase; a.row_cnt[g] = s_ncell;
    }
    pdl_sync();
#pragma unroll
    for (uint32_t s = 0; s < QJ_SLOTS; s++) {
        if (at[s] == Q_NONE) continue;
        const uint32_t i = s * QJ_T + threadIdx.x;
        const uint64_t o = s_cbase + at[s];
        a.st_score[o] = sc[s]; a.st_perc[o] = pc[s]; a.st_tr[o] = tc[s];
        a.st_col[o] = s_key[i]; a.st_first[o] = s_first[i];
    }
}

// The rows k_qb_join handed on, on the single query's dense tables in HBM (k_q_join_hbm: all zero / all-ones first between
// rows).  The tables are laid out for hbm_cols >= every query's columns, so rows of different queries share a workgroup's tables.
__global__ __launch_bounds__(QJ_T) void k_qb_join_hbm(QBJoinArgs b) {
    __shared__ QDesc s_d[QJ_T];
    __shared__ uint32_t s_cnt[QJ_T], s_pre[QJ_T + 1 + QJ_T / PDL_WAVE];
    __shared__ uint32_t s_stop, s_ntouch, s_ncell, s_emit;
    __shared__ unsigned long long s_cbase;
    const uint32_t n_cols = b.hbm_cols;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(b.a.hbm + (size_t) blockIdx.x * n_cols * 16);
    uint32_t *first = reinterpret_cast<uint32_t *>(acc + n_cols);
    uint32_t *touched = first + n_cols;
    const uint32_t n_over = (uint32_t) *b.a.n_overflow;
    for (uint32_t w = blockIdx.x; w < n_over; w += gridDim.x) {
        uint32_t g;
        const QJoinArgs a = qb_row_args(b, b.a.overflow_rows[w], g);
        if (threadIdx.x == 0) { s_stop = 0; s_ntouch = 0; s_ncell = 0; s_emit = 0; }
        pdl_sync();
        q_walk_row(a, g, s_d, s_cnt, s_pre, &s_stop, [&](uint32_t col, unsigned long long packed, uint32_t key) -> bool {
            const uint32_t old = atomicMin(&first[col], key);
            if (old == 0xffffffffu) touched[atomicAdd(&s_ntouch, 1u)] = col;
            atomicAdd(&acc[col], packed);
            return true;
        });
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        pdl_sync();
        const uint32_t nt = s_ntouch;
        for (uint32_t i = threadIdx.x; i < nt; i += QJ_T) {       // count (the maxima are taken here, once per cell)
            const uint32_t col = ld_agent(&touched[i]);
            float p, t;
            if (q_finalize(a, g, col, ld_agent(&acc[col]), p, t) > 0.0f) atomicAdd(&s_ncell, 1u);
        }
        pdl_sync();
        if (threadIdx.x == 0) {
            s_cbase = atomicAdd(a.cell_cursor, (unsigned long long) s_ncell);
            a.row_base[g] = (uint32_t) s_cbase; a.row_cnt[g] = s_ncell;
        }
        pdl_sync();
        const float threshold = 1.0f / (2.0f * (float) a.k);
        const uint32_t my_k = a.kseq_q[g];
        for (uint32_t i = threadIdx.x; i < nt; i += QJ_T) {       // write, and leave the entries clean
            const uint32_t col = ld_agent(&touched[i]);
            const unsigned long long v = ld_agent(&acc[col]);
            const uint32_t key = ld_agent(&first[col]);
            float p, t;
            const float score = finalize_cell(v, my_k, col < a.N ? a.kseq_b[col] : a.kseq_q[col - a.N], threshold, p, t);
            if (score > 0.0f) {
                const uint64_t o = s_cbase + atomicAdd(&s_emit, 1u);
                a.st_score[o] = score; a.st_perc[o] = p; a.st_tr[o] = t; a.st_col[o] = col; a.st_first[o] = key;
            }
            acc[col] = 0ull; first[col] = 0xffffffffu;
        }
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        pdl_sync();
    }
}

// cells of every query: the genes of a query are consecutive rows, so its cells are one stretch of the ordered cells
__global__ __launch_bounds__(64) void k_qb_counts(const uint32_t *fin_off, QBLayout lay, unsigned long long *ctl) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= lay.nq) return;
    const uint32_t g1 = lay.gene_begin[q + 1];
    const uint32_t end = g1 == lay.genes ? (uint32_t) ctl[QBG_EMITTED] : fin_off[g1];      // (fin_off holds the rows' starts; the scan's total closes it)
    qb_ctl(ctl, q)[QB_CTL_EMITTED] = end - fin_off[lay.gene_begin[q]];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct QBQuery {                    // what the host knows of one query before the device is asked
    uint32_t g0, n;                 // its genes in the caller's arrays
    uint64_t Rq, Mq;                // residues, k-mers
    uint64_t bytes;                 // device memory the stages before the join need for it (the chunking's weight)
};

template <class KeyT>
static QBView<KeyT> qb_view(pdl_ctx *c) {
    auto &w = c->qbb;
    QBView<KeyT> v;
    v.b.bkeys = c->keys_b.as<KeyT>(); v.b.brecpos = c->recpos.as<uint32_t>(); v.b.bvals = c->vals_b.as<uint32_t>(); v.b.post = c->post.as<uint2>();
    v.b.U = (uint32_t) c->U; v.b.M = c->M;
    v.b.qkeys = nullptr; v.b.qrecpos = nullptr; v.b.qpost = nullptr;
    v.srank = w.srank.as<KeyT>(); v.spost = w.spost.as<uint2>(); v.seg_off = w.seg_off.as<uint32_t>();
    return v;
}

// One chunk: queries [qa, qe) of `qs`.  Appends its blocks to out[qa..qe) / info (a failure leaves the freeing to the caller).
static void qb_run_chunk(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const std::vector<QBQuery> &qs, uint32_t qa, uint32_t qe,
                         uint32_t hbm_cols, pdl_scores *out, pdl_query_info *info, float *device_ms) {
    hipStream_t st = c->stream;
    auto &w = c->qbb;
    auto &sq = c->qb;                                             // the HBM tables and their bookkeeping are the single query's
    const uint32_t N = c->N, G = c->G, G1 = G + 1, k = c->rp.k;
    const uint32_t nq = qe - qa, ga = qs[qa].g0, NT = qs[qe - 1].g0 + qs[qe - 1].n - ga;
    const uint64_t r0 = offsets[ga], Rq = offsets[ga + NT] - r0;
    std::vector<uint64_t> h_off(NT + 1), h_koff(NT + 1), h_rbeg(nq + 1);
    std::vector<uint32_t> h_kseq(NT), h_gq(NT), h_gbeg(nq + 1);
    uint64_t Mq = 0;
    uint32_t n_max = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const QBQuery &Q = qs[qa + q];
        h_gbeg[q] = Q.g0 - ga; h_rbeg[q] = offsets[Q.g0] - r0;
        n_max = std::max(n_max, Q.n);
        for (uint32_t i = 0; i < Q.n; i++) {
            const uint32_t g = Q.g0 - ga + i;
            const uint64_t len = offsets[ga + g + 1] - offsets[ga + g];
            h_off[g] = offsets[ga + g] - r0; h_koff[g] = Mq;
            h_kseq[g] = len >= k ? (uint32_t) (len - k + 1) : 0u;      // (below 2^20: checked by the caller)
            h_gq[g] = q;
            Mq += h_kseq[g];
        }
    }
    h_off[NT] = Rq; h_koff[NT] = Mq; h_gbeg[nq] = NT; h_rbeg[nq] = Rq;
    for (int i = 0; i < 6; i++) if (!w.ev[i]) PDL_HIP(hipEventCreate(&w.ev[i]));
    int span = 0;
    auto span_begin = [&]() { PDL_HIP(hipEventRecord(w.ev[2 * span], st)); };
    auto span_end = [&]() { PDL_HIP(hipEventRecord(w.ev[2 * span + 1], st)); span++; };
    span_begin();

    // B-alpha (and the chunk on its way to the device)
    const size_t ctl_words = QBG_WORDS + (size_t) nq * QB_CTL_WORDS;
    w.ctl.alloc(ctl_words * sizeof(uint64_t));
    unsigned long long *ctl = w.ctl.as<unsigned long long>();
    PDL_HIP(hipMemsetAsync(ctl, 0, ctl_words * sizeof(uint64_t), st));
    w.res.alloc(Rq); w.off.alloc((NT + 1) * 8ull); w.koff.alloc((NT + 1) * 8ull); w.kseq.alloc(NT * 4ull);
    w.gene_begin.alloc((nq + 1) * 4ull); w.res_begin.alloc((nq + 1) * 8ull); w.gene_query.alloc(NT * 4ull);
    if (Rq) PDL_HIP(hipMemcpyAsync(w.res.p, residues + r0, Rq, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.off.p, h_off.data(), (NT + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.koff.p, h_koff.data(), (NT + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.kseq.p, h_kseq.data(), NT * 4ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.gene_begin.p, h_gbeg.data(), (nq + 1) * 4ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.res_begin.p, h_rbeg.data(), (nq + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.gene_query.p, h_gq.data(), NT * 4ull, hipMemcpyHostToDevice, st));
    const QBLayout lay{w.gene_begin.as<uint32_t>(), w.res_begin.as<uint64_t>(), w.gene_query.as<uint32_t>(), nq, NT};
    if (Rq) {
        QBAlphaArgs aa{};
        aa.res = w.res.as<uint8_t>(); aa.n = Rq; aa.lay = lay; aa.ctl = ctl;
        for (int b = 0; b < 256; b++) if (c->alpha_present[b]) aa.present[b >> 5] |= 1u << (b & 31);
        hipLaunchKernelGGL(k_qb_alpha, dim3((uint32_t) std::min<uint64_t>((Rq + 255) / 256, 1024)), dim3(256), 0, st, aa);
        PDL_HIP(hipGetLastError());
    }

    // B-dict, B-seg, B-fold, B-match, B-rows (sized by the bound Mq; the record count stays on the device until the look below)
    w.rowid.alloc(NT * 4ull);
    const uint32_t *rec_sorted = nullptr;
    if (Mq) {
        const size_t kb = c->key64 ? 8 : 4;
        w.keys_a.alloc(Mq * kb); w.keys_b.alloc(Mq * kb); w.vals_a.alloc(Mq * 4); w.vals_b.alloc(Mq * 4);
        w.recpos.alloc((Mq + 1) * 4); w.post.alloc(Mq * 8);
        const uint64_t *d_u = reinterpret_cast<const uint64_t *>(ctl + QBG_RECORDS);
        const void *qkeys = pdl_query_dictionary(c, w.res.as<uint8_t>(), w.off.as<uint64_t>(), w.koff.as<uint64_t>(), NT, Mq, Rq, w.keys_a.p, w.keys_b.p,
                                                 w.vals_a.as<uint32_t>(), w.vals_b.as<uint32_t>(), w.recpos.as<uint32_t>(), w.post.as<uint2>(),
                                                 reinterpret_cast<uint64_t *>(ctl + QBG_RECORDS));
        w.qkey.alloc(Mq * 8); w.perm.alloc(Mq * 8); w.srank.alloc(Mq * kb); w.spost.alloc(Mq * 8); w.seg_off.alloc((nq + 1) * 4ull);
        w.folds.alloc(nq * sizeof(QFold)); w.desc.alloc(Mq * sizeof(QDesc)); w.gkey.alloc(Mq * 8); w.rec_sorted.alloc(Mq * 8);
        w.row_lookups.alloc(NT * 4ull); w.row_off.alloc((NT + 1) * 4ull);
        PDL_HIP(hipMemsetAsync(w.row_lookups.p, 0, NT * 4ull, st));
        PDL_HIP(hipMemsetAsync(w.seg_off.p, 0, (nq + 1) * 4ull, st));
        const dim3 grid_m((uint32_t) ((Mq + 255) / 256));
        // every query's records as one segment, in (rank, gene) order: a stable sort of the record indices by query
        uint32_t *qk_in = w.qkey.as<uint32_t>(), *qk_out = qk_in + Mq;
        uint32_t *pm_in = w.perm.as<uint32_t>(), *pm_out = pm_in + Mq;
        hipLaunchKernelGGL(k_qb_seg_key, grid_m, dim3(256), 0, st, (const uint2 *) w.post.as<uint2>(), (const unsigned long long *) ctl, lay, qk_in);
        PDL_HIP(hipGetLastError());
        pdl_sort_pairs<uint32_t, uint32_t>(c, qk_in, qk_out, pm_in, pm_out, Mq, std::max<uint32_t>(1, bit_length64(nq)), true, d_u, 0, true);
        QBMatchOut mo{w.desc.as<QDesc>(), w.gkey.as<uint32_t>(), w.row_lookups.as<uint32_t>(), ctl};
        auto run = [&](auto key_tag) {
            using KeyT = decltype(key_tag);
            QBView<KeyT> v = qb_view<KeyT>(c);
            v.qid_sorted = qk_out;
            hipLaunchKernelGGL(k_qb_gather<KeyT>, grid_m, dim3(256), 0, st, static_cast<const KeyT *>(qkeys), (const uint32_t *) w.recpos.as<uint32_t>(),
                               (const uint2 *) w.post.as<uint2>(), (const uint32_t *) pm_out, (const uint32_t *) qk_out, (const unsigned long long *) ctl, lay,
                               w.srank.as<KeyT>(), w.spost.as<uint2>(), w.seg_off.as<uint32_t>());
            hipLaunchKernelGGL(k_qb_fold<KeyT>, dim3((nq + 63) / 64), dim3(64), 0, st, v, nq, ctl, w.folds.as<QFold>());
            hipLaunchKernelGGL(k_qb_match<KeyT>, grid_m, dim3(256), 0, st, v, (const QFold *) w.folds.as<QFold>(), lay, mo, Mq);
        };
        if (c->key64) run(uint64_t{}); else run(uint32_t{});
        PDL_HIP(hipGetLastError());
        // each gene's records in rank order: a stable sort of the segment positions by chunk gene
        uint32_t *gk_in = w.gkey.as<uint32_t>(), *gk_out = gk_in + Mq;
        uint32_t *ix_in = w.rec_sorted.as<uint32_t>(), *ix_out = ix_in + Mq;
        pdl_sort_pairs<uint32_t, uint32_t>(c, gk_in, gk_out, ix_in, ix_out, Mq, std::max<uint32_t>(1, bit_length64(NT)), true, d_u, 0, true);
        hipLaunchKernelGGL(k_qb_row_off, dim3((NT + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t *) gk_out, ctl, lay, N, w.row_off.as<uint32_t>(),
                           (const uint32_t *) w.row_lookups.as<uint32_t>(), QJ_LIMIT, w.rowid.as<uint32_t>());
        PDL_HIP(hipGetLastError());
        rec_sorted = ix_out;
    }
    std::vector<uint64_t> h_ctl(ctl_words);
    span_end();
    {
        PinRead rd(c);
        const uint64_t *pc = rd.add<uint64_t>(ctl, ctl_words);
        rd.sync();
        memcpy(h_ctl.data(), pc, ctl_words * sizeof(uint64_t));
    }
    auto hq = [&](uint32_t q, uint32_t word) -> uint64_t { return h_ctl[QBG_WORDS + (size_t) q * QB_CTL_WORDS + word]; };
    for (uint32_t q = 0; q < nq; q++)
        if (hq(q, QB_CTL_BAD_BYTE)) {
            char who[48];
            snprintf(who, sizeof(who), "query %u:", qa + q);
            pdl_fail_absent_byte(hq(q, QB_CTL_BAD_BYTE), who);
        }
    span_begin();
    const uint64_t Ut = h_ctl[QBG_RECORDS];
    uint64_t bound = 0, may_overflow = 0;
    for (uint32_t q = 0; q < nq; q++) { bound += hq(q, QB_CTL_BOUND); may_overflow += hq(q, QB_CTL_MAY_OVERFLOW); }
    if (bound >= 0xffffffffull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "%llu candidate cells exceed 32-bit cell positions", (unsigned long long) bound);

    // B-join, B-order
    const size_t ms_floats = (size_t) NT * G1, cm_floats = (size_t) nq * N + NT;
    w.MS.alloc(ms_floats * 4); w.CM.alloc(cm_floats * 4);
    PDL_HIP(hipMemsetAsync(w.MS.p, 0, ms_floats * 4, st));
    PDL_HIP(hipMemsetAsync(w.CM.p, 0, cm_floats * 4, st));
    const uint64_t cap = std::max<uint64_t>(bound, 1);
    uint64_t Z = 0;
    if (Ut) {
        w.row_base.alloc(NT * 4ull); w.row_cnt.alloc(NT * 4ull); w.fin_off.alloc((NT + 1) * 4ull); w.overflow.alloc(NT * 4ull);
        w.st.alloc(cap * 20); w.cells.alloc(cap * 20);
        QBJoinArgs b{};
        QJoinArgs &a = b.a;
        b.lay = lay; b.hbm_cols = hbm_cols;
        a.post = c->post.as<uint2>(); a.qpost = w.spost.as<uint2>(); a.desc = w.desc.as<QDesc>();
        a.rec_sorted = rec_sorted; a.row_off = w.row_off.as<uint32_t>();
        a.kseq_b = c->kseq_len.as<uint32_t>(); a.kseq_q = w.kseq.as<uint32_t>(); a.genome_b = c->d_gen;
        a.N = N; a.n = 0; a.G1 = G1; a.k = k;
        a.MS = w.MS.as<float>(); a.CM = w.CM.as<float>();
        a.row_base = w.row_base.as<uint32_t>(); a.row_cnt = w.row_cnt.as<uint32_t>();
        float *stf = w.st.as<float>();
        a.st_score = stf; a.st_perc = stf + cap; a.st_tr = stf + 2 * cap;
        a.st_col = reinterpret_cast<uint32_t *>(stf + 3 * cap); a.st_first = reinterpret_cast<uint32_t *>(stf + 4 * cap);
        a.cell_cursor = ctl + QBG_CELL_CURSOR; a.overflow_rows = w.overflow.as<uint32_t>(); a.n_overflow = ctl + QBG_OVERFLOW_ROWS;
        hipLaunchKernelGGL(k_qb_join, dim3(NT), dim3(QJ_T), 0, st, b);
        PDL_HIP(hipGetLastError());
        if (may_overflow) {      // some row has more lookups than the LDS table holds keys: did it leave the table?
            uint64_t n_over = 0;
            span_end();
            {
                PinRead rd(c);
                const uint64_t *pc = rd.add<uint64_t>(ctl + QBG_OVERFLOW_ROWS, 1);
                rd.sync();
                n_over = pc[0];
            }
            span_begin();
            if (n_over) {
                // the single query's tables (pdl_query.h), laid out for the batch's widest union: clean tables of exactly that
                // layout are taken as they are, others are cleared — and the bookkeeping says what a later query will find
                const uint32_t W = (uint32_t) std::min<uint64_t>(n_over, QH_WG);
                if (!sq.hbm_clean || sq.hbm_cols != hbm_cols || sq.hbm_slots < W) {
                    sq.hbm_clean = false;
                    sq.hbm.alloc((size_t) W * hbm_cols * 16);
                    hipLaunchKernelGGL(k_q_hbm_clear, dim3((uint32_t) std::min<uint64_t>(((uint64_t) W * hbm_cols + 255) / 256, 4096)), dim3(256), 0, st,
                                       sq.hbm.as<uint8_t>(), hbm_cols, W);
                    sq.hbm_cols = hbm_cols; sq.hbm_slots = W; sq.hbm_clean = true;
                }
                a.hbm = sq.hbm.as<uint8_t>();
                hipLaunchKernelGGL(k_qb_join_hbm, dim3(W), dim3(QJ_T), 0, st, b);
                PDL_HIP(hipGetLastError());
            }
        }
        scan_and_apply(c, NT, RowCntFlag{w.row_cnt.as<uint32_t>(), nullptr}, FinOffApply{w.fin_off.as<uint32_t>()}, reinterpret_cast<uint64_t *>(ctl + QBG_EMITTED));
        OrderArgs o{};
        o.row_base = a.row_base; o.row_cnt = a.row_cnt; o.fin_off = w.fin_off.as<uint32_t>(); o.task_rows = w.rowid.as<uint32_t>();
        o.st_score = a.st_score; o.st_perc = a.st_perc; o.st_tr = a.st_tr; o.st_col = a.st_col; o.st_first = a.st_first;
        float *cf = w.cells.as<float>();
        o.c_score = cf; o.c_perc = cf + cap; o.c_tr = cf + 2 * cap;
        o.c_row = reinterpret_cast<int32_t *>(cf + 3 * cap); o.c_col = reinterpret_cast<int32_t *>(cf + 4 * cap);
        o.n_rows = NT; o.canonical = (c->flags & PDL_FLAG_CANONICAL_ORDER) ? 1u : 0u; o.pack_ok = (uint64_t) N + n_max < (1u << 22) ? 1u : 0u;
        o.wide_rows = reinterpret_cast<uint32_t *>(ctl + QBG_WIDE_ROWS);
        const uint32_t cus = (uint32_t) pdl_cus(c);
        hipLaunchKernelGGL(k_order_rows_wave, dim3((NT + 3) / 4), dim3(256), 0, st, o);
        hipLaunchKernelGGL(k_order_rows, dim3(std::min<uint32_t>(NT, cus * 8)), dim3(ORDER_THREADS), 0, st, o);
        hipLaunchKernelGGL(k_qb_counts, dim3((nq + 63) / 64), dim3(64), 0, st, (const uint32_t *) w.fin_off.as<uint32_t>(), lay, ctl);
        PDL_HIP(hipGetLastError());
        span_end();
        {
            PinRead rd(c);                                       // the per-query counts (and the cursors beside them): one read
            const uint64_t *pc = rd.add<uint64_t>(ctl, ctl_words);
            rd.sync();
            memcpy(h_ctl.data(), pc, ctl_words * sizeof(uint64_t));
        }
        const uint64_t staged = h_ctl[QBG_CELL_CURSOR];
        Z = h_ctl[QBG_EMITTED];
        if (Z > bound || staged > bound) PDL_FAIL(PDL_ERR_DEVICE, "query batch join: %llu cells staged, bound %llu", (unsigned long long) staged, (unsigned long long) bound);
    } else {
        span_end();
    }

    // B-copy: the chunk's cells and maxima come over in one piece each (7 copies per chunk, not per query) into pinned host
    // memory — a DMA, no staging by the runtime — then every query's block is cut out on the host
    const size_t stage_words = (size_t) Z * 5 + ms_floats + cm_floats;
    if (w.stage_bytes < stage_words * 4) {
        if (w.stage) { (void) hipHostFree(w.stage); w.stage = nullptr; w.stage_bytes = 0; }
        PDL_HIP(hipHostMalloc((void **) &w.stage, stage_words * 4 + (stage_words * 4) / 4, hipHostMallocDefault));
        w.stage_bytes = stage_words * 4 + (stage_words * 4) / 4;
    }
    const uint32_t *h_cells = reinterpret_cast<const uint32_t *>(w.stage);
    const float *h_ms = reinterpret_cast<const float *>(w.stage) + (size_t) Z * 5, *h_cm = h_ms + ms_floats;
    if (Z) {
        const float *cf = w.cells.as<float>();
        for (int i = 0; i < 5; i++) PDL_HIP(hipMemcpyAsync(w.stage + (size_t) i * Z * 4, cf + (size_t) i * cap, Z * 4, hipMemcpyDeviceToHost, st));
    }
    PDL_HIP(hipMemcpyAsync(const_cast<float *>(h_ms), w.MS.p, ms_floats * 4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipMemcpyAsync(const_cast<float *>(h_cm), w.CM.p, cm_floats * 4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipStreamSynchronize(st));
    float ms_total = 0.f;
    for (int i = 0; i < span; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, w.ev[2 * i], w.ev[2 * i + 1]) == hipSuccess) ms_total += ms;
    }
    *device_ms += ms_total;
    auto xm = [](size_t bytes) { void *p = malloc(bytes ? bytes : 1); if (!p) throw std::bad_alloc(); return p; };
    uint64_t z0 = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const QBQuery &Q = qs[qa + q];
        const uint64_t Zq = Ut ? hq(q, QB_CTL_EMITTED) : 0;
        const uint32_t n = Q.n, NC = N + n;
        if (z0 + Zq > Z) PDL_FAIL(PDL_ERR_DEVICE, "query batch: the queries' cells (%llu) pass the emitted total %llu", (unsigned long long) (z0 + Zq), (unsigned long long) Z);
        pdl_scores &r = out[qa + q];                             // (filled in place: a throw leaves what is allocated to the caller's pdl_free_scores)
        r.scoresCount = (uint32_t) Zq; r.rows = n; r.genomes = G1; r.sequences = NC;
        r.scores = (float *) xm(Zq * 4); r.percs = (float *) xm(Zq * 4); r.tr_percs = (float *) xm(Zq * 4);
        r.row = (int32_t *) xm(Zq * 4); r.column = (int32_t *) xm(Zq * 4);
        r.first_seq_genome = (int32_t *) xm(Zq * 4); r.second_seq_genome = (int32_t *) xm(Zq * 4);
        r.max_genome_score = (float *) xm((size_t) n * G1 * 4); r.max_genome_score_col = (float *) xm((size_t) NC * 4);
        r.scoresMaxMappings = (int32_t *) xm((size_t) NC * 4);
        void *dst[5] = {r.scores, r.percs, r.tr_percs, r.row, r.column};
        for (int i = 0; i < 5; i++) if (Zq) memcpy(dst[i], h_cells + (size_t) i * Z + z0, Zq * 4);
        memcpy(r.max_genome_score, h_ms + (size_t) h_gbeg[q] * G1, (size_t) n * G1 * 4);
        memcpy(r.max_genome_score_col, h_cm + (size_t) q * N + h_gbeg[q], (size_t) NC * 4);
        for (uint64_t i = 0; i < Zq; i++) {
            r.first_seq_genome[i] = (int32_t) G;
            const uint32_t col = (uint32_t) r.column[i];
            r.second_seq_genome[i] = col < N ? (int32_t) c->h_genome_of[col] : (int32_t) G;
        }
        for (uint32_t i = 0; i < N; i++) r.scoresMaxMappings[i] = 0x7fffffff;
        for (uint32_t g = 0; g < n; g++) r.scoresMaxMappings[N + g] = (int32_t) g;
        z0 += Zq;
        if (info) {
            pdl_query_info &fi = info[qa + q];
            memset(&fi, 0, sizeof(fi));
            fi.residues = Q.Rq; fi.kmer_occurrences = Q.Mq; fi.records = hq(q, QB_CTL_RECORDS); fi.matched_records = hq(q, QB_CTL_MATCHED);
            fi.genome_cost = hq(q, QB_CTL_COST);
            fi.device_ms = ms_total / (float) nq;
        }
    }
}

void pdl_run_query_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                         pdl_scores *out, pdl_query_info *info, pdl_query_batch_info *binfo) {
    const uint32_t N = c->N, G1 = c->G + 1, k = c->rp.k;
    if (c->R + (offsets[n] - offsets[0]) >= 0xfffffff0ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 residues in the base and the batch need 64-bit stream positions");
    if (c->max_kseq >= (1ull << 20)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "a base gene of %llu k-mers: queries need genes below 2^20 k-mers", (unsigned long long) c->max_kseq);
    const size_t kb = c->key64 ? 8 : 4;
    std::vector<QBQuery> qs(n_queries);
    uint32_t n_max = 0;
    for (uint32_t q = 0; q < n_queries; q++) {
        QBQuery &Q = qs[q];
        Q.g0 = gene_begin[q]; Q.n = gene_begin[q + 1] - gene_begin[q];
        Q.Rq = offsets[Q.g0 + Q.n] - offsets[Q.g0]; Q.Mq = 0;
        for (uint32_t g = Q.g0; g < Q.g0 + Q.n; g++) {
            const uint64_t len = offsets[g + 1] - offsets[g];
            const uint64_t ks = len >= k ? len - k + 1 : 0;
            if (ks >= (1u << 20)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "query %u: gene %u has %llu k-mers: queries need genes below 2^20 k-mers", q, g - Q.g0, (unsigned long long) ks);
            Q.Mq += ks;
        }
        if (Q.Mq >= 0x7ffff000ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "query %u: %llu k-mers exceed the 31-bit record positions", q, (unsigned long long) Q.Mq);
        // what the stages hold per k-mer (two key and value halves, recpos, postings, the two index sorts, segment copies, group
        // descriptions) and per gene / column (maxima, row tables); staging and cells are sized once the match has counted them
        Q.bytes = Q.Rq + Q.Mq * (3 * kb + 2 * 4 + 4 + 8 + 4 * 8 + 8 + sizeof(QDesc)) + ((uint64_t) N + Q.n) * 4 + (uint64_t) Q.n * (G1 * 4ull + 48);
        n_max = std::max(n_max, Q.n);
    }
    const uint32_t hbm_cols = N + n_max;
    // chunks of consecutive queries within the byte budget (and the 31-bit record positions); one query always goes
    float device_ms = 0.f;
    uint32_t chunks = 0;
    for (uint32_t qa = 0; qa < n_queries;) {
        uint32_t qe = qa + 1;
        uint64_t bytes = qs[qa].bytes, m = qs[qa].Mq;
        while (qe < n_queries && bytes + qs[qe].bytes <= c->opt_query_batch_bytes && m + qs[qe].Mq < 0x7ffff000ull) { bytes += qs[qe].bytes; m += qs[qe].Mq; qe++; }
        qb_run_chunk(c, residues, offsets, qs, qa, qe, hbm_cols, out, info, &device_ms);
        chunks++;
        qa = qe;
    }
    if (binfo) { binfo->queries = n_queries; binfo->chunks = chunks; binfo->device_ms = device_ms; }
}
