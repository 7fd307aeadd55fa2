// pdl_query_batch.h — K-query for a batch: q new genomes scored against the dictionary that is already in HBM, each on its own
// (pdl_query_batch, include/pandelos_amd.h), included from pdl_join.hip behind pdl_query.h.  The fold (q_fold_base,
// q_fold_union), the group description (q_describe) and the row program (q_row_lds, q_row_hbm) are the single query's: the kernels
// here give them a query's segment and a row's own arguments.  So are the host's stages — q_dictionary, q_match_out, q_gene_rows,
// q_join_and_order over c->qbb as QStageBufs —, the control words (Q_RUN_*, Q_QRY_*) and the result view (pdl_query_cells):
// pdl_run_query_chunk_device keeps what is a chunk's own, the staging, the verdicts of option "query_rekey", B-seg, and its launches.
//
// Contract: block j is what pdl_query_scores returns for genome j alone — computeScores(G) of base + genome j.  The queries
// never see each other; the base context is only read.
//
// One genome cannot fill the chip (the match is one round of latency, the join has fewer workgroups than the chip
// holds, the launches and host reads are a third of the time), so the stages run ONCE over all genes of a chunk of queries:
//
//   B-stage  qb_stage_chunk the chunk's layout, its control words cleared, residues and the six layout arrays on their way up
//   B-alpha  k_q_absent<.., BATCH> (pdl_query.h)   every query byte against the base's letters; per query the smallest absent byte
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
//   B-copy   the chunk's cells and maxima to the host in one piece each, every query's block cut out there
//
// B-alpha .. B-order and the per-query counts are pdl_run_query_chunk_device: the cells stay in HBM (pdl_query_cells).  pdl_query_batch follows
// it with B-copy; K-place for a batch (pdl_place_batch.h) filters the cells where they lie instead.
//
// Fold and match run over one view, QBView<KeyB, KeyQ, RK> (QView's accessors over segment positions), chosen by q_with_keys.
//
// Option "query_rekey": behind B-stage comes qb_rekey_chunk — every query's absent bytes (k_q_absent<LETTERS, BATCH>), the host's
// verdict per query and the chunk's joint alphabet, the chunk cut where that would not be exact: what is staged serves the prefix
// as it is, only the counts are taken again.  A chunk whose queries bring a letter is ranked once with the joint table, B-seg
// copies those keys, Q-rebase (pdl_rekey.h) runs over the segment positions and k_qb_fold / k_qb_match <KeyB, KeyQ, true> take its
// output as the single query's do.  A chunk without a new letter takes the stages above untouched.
//
// Positions of query records (QDesc.qlo/qhi/qextra, QFold.qL) are positions in the segmented arrays of the chunk; QDesc.key is
// taken relative to the segment start, so it is the single query's key.
#pragma once
#include "pdl_query.h"

// (the chunk's control words, qbb.ctl: Q_RUN_* for the chunk, Q_QRY_* per query — pdl_query.h)

// the chunk's layout: genes [gene_begin[q], gene_begin[q + 1]) and bytes [res_begin[q], res_begin[q + 1]) belong to query q
struct QBLayout {
    const uint32_t *gene_begin;     // [nq + 1]
    const uint64_t *res_begin;      // [nq + 1]
    const uint32_t *gene_query;     // [genes]
    uint32_t nq, genes;
};

// key of the segment sort: the query of every record of the chunk's dictionary
__global__ __launch_bounds__(256) void k_qb_seg_key(const uint2 *post, const unsigned long long *ctl, QBLayout lay, uint32_t *key) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u < (uint32_t) ctl[Q_RUN_RECORDS]) key[u] = lay.gene_query[post[u].x];
}

// Records in segment order: rank and {local gene, count} of position j, and seg_off[q] = first position of query q (a query
// without records gets an empty segment; seg_off was cleared, which is right for a chunk without records).
template <class KeyT>
__global__ __launch_bounds__(256) void k_qb_gather(const KeyT *keys, const uint32_t *recpos, const uint2 *post, const uint32_t *perm,
                                                   const uint32_t *qid_sorted, const unsigned long long *ctl, QBLayout lay,
                                                   KeyT *srank, uint2 *spost, uint32_t *seg_off) {
    const uint32_t U = (uint32_t) ctl[Q_RUN_RECORDS];
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

// The chunk's records as fold and match see them (QView's accessors, pdl_query.h, over segment positions).  Option "query_rekey", a
// chunk whose queries bring letters the base lacks (RK): the chunk is ranked once, in the base's letters plus those of ALL its
// queries (a block is the same in whichever exact superset alphabet it was ranked); srank holds those keys, of type KeyQ, and r
// what Q-rebase left for every segment position.
template <class KeyB, class KeyQ, bool RK> struct QBView : QRebasedIf<KeyB, RK> {
    QBase<KeyB> b;
    const KeyQ *srank; const uint2 *spost;
    const uint32_t *seg_off, *qid_sorted;
    __device__ unsigned long long qrank(uint32_t i) const { return (unsigned long long) srank[i]; }
    __device__ unsigned long long bkey(uint32_t i, bool &none) const {
        if constexpr (RK) { none = this->r.none[i] != 0; return (unsigned long long) this->r.bkey[i]; }
        else { none = false; return qrank(i); }
    }
    __device__ const unsigned long long *up3() const { if constexpr (RK) return this->r.up3; else return nullptr; }
};

// One thread per query: the base's fold (the same for all, computed by each) and the union's with this query's largest rank.
template <class KeyB, class KeyQ, bool RK>
__global__ __launch_bounds__(64) void k_qb_fold(QBView<KeyB, KeyQ, RK> v, uint32_t nq, unsigned long long *ctl, QFold *out) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const uint32_t s0 = v.seg_off[q], s1 = v.seg_off[q + 1];
    q_query_ctl(ctl, q)[Q_QRY_RECORDS] = s1 - s0;
    if (s0 == s1) {                                               // no k-mer: no record reads the fold
        QFold f{};
        f.p = Q_NONE; f.qL = Q_NONE;
        out[q] = f;
        return;
    }
    bool lonely, has_r2;
    QFold f = q_fold_base(v.b, lonely, has_r2, v.up3());
    q_fold_union(f, lonely, has_r2, v, s0, s1);
    out[q] = f;
}

// One thread per record of the chunk: k_q_match inside the record's own segment; cost and matched count per query
template <class KeyB, class KeyQ, bool RK>
__global__ __launch_bounds__(256) void k_qb_match(QBView<KeyB, KeyQ, RK> v, const QFold *folds, QBLayout lay, QMatchOut o, uint64_t bound) {
    const uint32_t Ut = (uint32_t) o.ctl[Q_RUN_RECORDS];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    unsigned long long cost = 0, matched = 0;
    uint32_t q = Q_NONE;
    if (j < Ut && j < bound) {
        q = v.qid_sorted[j];
        const QFold f = folds[q];
        const QDesc d = q_describe(f, v, j, v.seg_off[q], v.seg_off[q + 1]);
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
    if (cost) atomicAdd(q_query_ctl(o.ctl, q) + Q_QRY_COST, cost);
    if (matched) atomicAdd(q_query_ctl(o.ctl, q) + Q_QRY_MATCHED, matched);
}

// row_off[g] = first position of chunk gene g in the gene-sorted records; per query: staging bound = sum of
// min(lookups, columns of ITS union), rows whose lookups exceed `limit`; rowid[g] = the gene's id in its union
__global__ __launch_bounds__(256) void k_qb_row_off(const uint32_t *gene_sorted, unsigned long long *ctl, QBLayout lay, uint32_t N, uint32_t *row_off,
                                                    const uint32_t *row_lookups, uint32_t limit, uint32_t *rowid) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    const uint32_t Ut = (uint32_t) ctl[Q_RUN_RECORDS];
    if (g > lay.genes) return;
    uint32_t lo = 0, hi = Ut;
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (gene_sorted[m] < g) lo = m + 1; else hi = m; }
    row_off[g] = lo;
    if (g == lay.genes) return;
    const uint32_t q = lay.gene_query[g], g0 = lay.gene_begin[q];
    rowid[g] = N + (g - g0);
    const uint32_t n_cols = N + (lay.gene_begin[q + 1] - g0), l = row_lookups[g];
    if (l) atomicAdd(q_query_ctl(ctl, q) + Q_QRY_BOUND, (unsigned long long) min(l, n_cols));
    if (l > limit) atomicAdd(q_query_ctl(ctl, q) + Q_QRY_MAY_OVERFLOW, 1ull);
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
    uint32_t g;
    const QJoinArgs a = qb_row_args(b, blockIdx.x, g);
    q_row_lds(a, g, blockIdx.x);                                  // (overflow id = the chunk gene: k_qb_join_hbm cuts its query's slices out again)
}

// The rows k_qb_join handed on.  The tables are laid out for hbm_cols >= every query's columns, so rows of different queries
// share a workgroup's tables.
__global__ __launch_bounds__(QJ_T) void k_qb_join_hbm(QBJoinArgs b) {
    const uint32_t n_cols = b.hbm_cols;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(b.a.hbm + (size_t) blockIdx.x * n_cols * 16);
    uint32_t *first = reinterpret_cast<uint32_t *>(acc + n_cols);
    const uint32_t n_over = (uint32_t) *b.a.n_overflow;
    for (uint32_t w = blockIdx.x; w < n_over; w += gridDim.x) {
        uint32_t g;
        const QJoinArgs a = qb_row_args(b, b.a.overflow_rows[w], g);
        q_row_hbm(a, g, acc, first, first + n_cols);
    }
}

// cells of every query: the genes of a query are consecutive rows, so its cells are one stretch of the ordered cells
__global__ __launch_bounds__(64) void k_qb_counts(const uint32_t *fin_off, QBLayout lay, unsigned long long *ctl) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= lay.nq) return;
    const uint32_t g1 = lay.gene_begin[q + 1];
    const uint32_t end = g1 == lay.genes ? (uint32_t) ctl[Q_RUN_EMITTED] : fin_off[g1];      // (fin_off holds the rows' starts; the scan's total closes it)
    q_query_ctl(ctl, q)[Q_QRY_EMITTED] = end - fin_off[lay.gene_begin[q]];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
template <class KeyB, class KeyQ, bool RK>
static QBView<KeyB, KeyQ, RK> qb_view(pdl_ctx *c, const uint32_t *qid_sorted) {
    auto &w = c->qbb;
    QBView<KeyB, KeyQ, RK> v;
    v.b = q_base<KeyB>(c);
    v.srank = w.srank.as<KeyQ>(); v.spost = w.spost.as<uint2>(); v.seg_off = w.seg_off.as<uint32_t>(); v.qid_sorted = qid_sorted;
    if constexpr (RK) v.r = q_rebased<KeyB>(c);
    return v;
}

// A chunk as the host lays it out and qb_stage_chunk leaves it in c->qbb: the counts, and the host's copies of the seven arrays
// (off, koff, kseq by chunk gene; gene_query; gene_begin, res_begin by query) for as long as their uploads may read them.
struct QBStage {
    uint32_t nq = 0, NT = 0, n_max = 0;             // queries, genes, genes of the largest query
    uint64_t Rq = 0, Mq = 0;                        // residues, k-mers
    std::vector<uint64_t> off, koff, rbeg;
    std::vector<uint32_t> kseq, gq, gbeg;
    size_t ctl_words() const { return q_ctl_words(nq); }
    // The counts of the first n queries [qa, qa + n).  Every staged array is valid as a prefix — off[NT'] = Rq', koff[NT'] = Mq',
    // gene_begin[n] = NT', res_begin[n] = Rq', the control words lie query by query — so a chunk that is cut stages nothing again.
    void take(const std::vector<QBQuery> &qs, uint32_t qa, uint32_t n) {
        nq = n; NT = gbeg[n]; Rq = rbeg[n]; Mq = koff[NT];
        n_max = 0;
        for (uint32_t q = 0; q < n; q++) n_max = std::max(n_max, qs[qa + q].n);
    }
};
// The queries [qa, qe) on their way to the device: the layout, the chunk's control words cleared, the seven uploads.  Opens the
// chunk's first stretch of device work (w.spans) behind the host's layout.
static QBStage qb_stage_chunk(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const std::vector<QBQuery> &qs, uint32_t qa, uint32_t qe) {
    hipStream_t st = c->stream;
    auto &w = c->qbb;
    const uint32_t k = c->rp.k, nq = qe - qa, ga = qs[qa].g0, NT = qs[qe - 1].g0 + qs[qe - 1].n - ga;
    const uint64_t r0 = offsets[ga], Rq = offsets[ga + NT] - r0;
    QBStage s;
    s.off.resize(NT + 1); s.koff.resize(NT + 1); s.rbeg.resize(nq + 1); s.kseq.resize(NT); s.gq.resize(NT); s.gbeg.resize(nq + 1);
    uint64_t Mq = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const QBQuery &Q = qs[qa + q];
        s.gbeg[q] = Q.g0 - ga; s.rbeg[q] = offsets[Q.g0] - r0;
        for (uint32_t i = 0; i < Q.n; i++) {
            const uint32_t g = Q.g0 - ga + i;
            const uint64_t len = offsets[ga + g + 1] - offsets[ga + g];
            s.off[g] = offsets[ga + g] - r0; s.koff[g] = Mq;
            s.kseq[g] = len >= k ? (uint32_t) (len - k + 1) : 0u;      // (below 2^20: checked by the caller)
            s.gq[g] = q;
            Mq += s.kseq[g];
        }
    }
    s.off[NT] = Rq; s.koff[NT] = Mq; s.gbeg[nq] = NT; s.rbeg[nq] = Rq;
    s.take(qs, qa, nq);
    w.spans.start(st);
    w.spans.begin();
    w.ctl.alloc(s.ctl_words() * sizeof(uint64_t));
    PDL_HIP(hipMemsetAsync(w.ctl.p, 0, s.ctl_words() * sizeof(uint64_t), st));
    w.res.alloc(Rq); w.off.alloc((NT + 1) * 8ull); w.koff.alloc((NT + 1) * 8ull); w.kseq.alloc(NT * 4ull);
    w.gene_begin.alloc((nq + 1) * 4ull); w.res_begin.alloc((nq + 1) * 8ull); w.gene_query.alloc(NT * 4ull);
    if (Rq) PDL_HIP(hipMemcpyAsync(w.res.p, residues + r0, Rq, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.off.p, s.off.data(), (NT + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.koff.p, s.koff.data(), (NT + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.kseq.p, s.kseq.data(), NT * 4ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.gene_begin.p, s.gbeg.data(), (nq + 1) * 4ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.res_begin.p, s.rbeg.data(), (nq + 1) * 8ull, hipMemcpyHostToDevice, st));
    PDL_HIP(hipMemcpyAsync(w.gene_query.p, s.gq.data(), NT * 4ull, hipMemcpyHostToDevice, st));
    return s;
}

// Option "query_rekey", behind the staging of a chunk [qa, qa + s.nq): every query's letters come to the host (the absent-byte scan
// over the chunk's bytes), and the host decides.  Each query's own verdict uses its own union only (q_rekey_verdict: a refusal names
// the first such query).  The chunk is ranked with the base's letters plus those of all its queries if that alphabet is exact;
// where a query tips it over, the chunk is cut in front of it (a chunk of one is a query's own union: exact, or refused): `s`
// then holds the counts of that prefix of what is staged.  rekey: the chunk's queries bring a letter and the plan for their joint
// letters is in c->qb.rk.  The scan closes the chunk's first stretch of device work; the next one is opened behind the verdicts.
static void qb_rekey_chunk(pdl_ctx *c, const std::vector<QBQuery> &qs, uint32_t qa, QBStage &s, bool &rekey) {
    auto &w = c->qbb;
    rekey = false;
    if (!s.Rq) return;
    unsigned long long *ctl = w.ctl.as<unsigned long long>();
    q_scan_absent<true, true>(c, w.res.as<uint8_t>(), s.Rq, w.res_begin.as<uint64_t>(), s.nq, Q_QRY_WORDS, ctl + Q_RUN_WORDS + Q_QRY_LETTERS);
    QCtlHost h(s.nq);
    h.read(c, w.spans, ctl, false);
    uint32_t joint[8] = {};
    const char *why = "";
    const bool base_exact = pdl_query_rekey_base_exact(c, &why);
    for (uint32_t q = 0; q < s.nq; q++) {
        uint32_t own[8], with[8];
        memcpy(own, q_query_ctl(h.w.data(), q) + Q_QRY_LETTERS, sizeof(own));
        if (!q_any_letter(own)) continue;
        bool grows = false;
        for (int i = 0; i < 8; i++) { with[i] = joint[i] | own[i]; grows = grows || with[i] != joint[i]; }
        if (q > 0 && grows && base_exact && !pdl_query_rekey_plan(c, with, false, &why)) { s.take(qs, qa, q); break; }
        char who[48];
        snprintf(who, sizeof(who), "query %u:", qa + q);
        q_rekey_verdict(c, own, who, false);
        memcpy(joint, with, sizeof(joint));
    }
    if (q_any_letter(joint)) {
        if (!pdl_query_rekey_plan(c, joint, true, &why)) PDL_FAIL(PDL_ERR_DEVICE, "query batch: the chunk's joint alphabet is not exact (%s)", why);
        rekey = true;
    }
    w.spans.begin();
}

// The device half of one chunk, queries [qa, qe) of `qs` — with option "query_rekey" a prefix of them (qb_rekey_chunk), the
// chunk's nq says how many: B-alpha ... B-order and the per-query counts.  The ordered cells, MS and CM stay in HBM.
pdl_query_cells pdl_run_query_chunk_device(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const std::vector<QBQuery> &qs, uint32_t qa, uint32_t qe,
                                           uint32_t hbm_cols) {
    hipStream_t st = c->stream;
    auto &w = c->qbb;

    // B-alpha (and the chunk on its way to the device)
    QBStage s = qb_stage_chunk(c, residues, offsets, qs, qa, qe);
    bool rekey = false;
    if (c->opt_query_rekey) qb_rekey_chunk(c, qs, qa, s, rekey);
    const uint32_t N = c->N, nq = s.nq, NT = s.NT;
    const uint64_t Mq = s.Mq;
    unsigned long long *ctl = w.ctl.as<unsigned long long>();
    const QBLayout lay{w.gene_begin.as<uint32_t>(), w.res_begin.as<uint64_t>(), w.gene_query.as<uint32_t>(), nq, NT};
    // (a chunk that is re-keyed has had its verdicts)
    if (!rekey) q_scan_absent<false, true>(c, w.res.as<uint8_t>(), s.Rq, lay.res_begin, nq, Q_QRY_WORDS, q_query_ctl(ctl, 0) + Q_QRY_BAD_BYTE);
    // (tables laid out for the batch's widest union, which every query's columns fit)
    const QRun run{NT, nq, s.gbeg.data(), lay.gene_begin, s.Rq, Mq, (uint64_t) N + s.n_max, hbm_cols, rekey, "query batch", qa};

    // B-dict, B-seg, B-fold, B-match, B-rows (sized by the bound Mq; the record count stays on the device until the look behind them)
    w.rowid.alloc(NT * 4ull);
    const uint32_t *rec_sorted = nullptr;
    if (Mq) {
        const uint64_t *d_u = reinterpret_cast<const uint64_t *>(ctl + Q_RUN_RECORDS);
        const void *qkeys = q_dictionary(c, w, run);
        w.qkey.alloc(Mq * 8); w.perm.alloc(Mq * 8); w.srank.alloc(Mq * q_key_bytes(c, rekey)); w.spost.alloc(Mq * 8); w.seg_off.alloc((nq + 1) * 4ull);
        w.folds.alloc(nq * sizeof(QFold));
        const QMatchOut mo = q_match_out(c, w, run);
        PDL_HIP(hipMemsetAsync(w.seg_off.p, 0, (nq + 1) * 4ull, st));
        const dim3 grid_m((uint32_t) ((Mq + 255) / 256));
        // every query's records as one segment, in (rank, gene) order: a stable sort of the record indices by query
        uint32_t *qk_in = w.qkey.as<uint32_t>(), *qk_out = qk_in + Mq;
        uint32_t *pm_in = w.perm.as<uint32_t>(), *pm_out = pm_in + Mq;
        hipLaunchKernelGGL(k_qb_seg_key, grid_m, dim3(256), 0, st, (const uint2 *) w.post.as<uint2>(), (const unsigned long long *) ctl, lay, qk_in);
        PDL_HIP(hipGetLastError());
        pdl_sort_pairs<uint32_t, uint32_t>(c, qk_in, qk_out, pm_in, pm_out, Mq, std::max<uint32_t>(1, bit_length64(nq)), true, d_u, 0, true);
        // the segments in the alphabet the chunk is ranked in; re-keyed: Q-rebase over the segment positions, fold and match in two alphabets
        q_with_keys(c, rekey, [&](auto key_b, auto key_q, auto rk) {
            using KeyB = decltype(key_b);
            using KeyQ = decltype(key_q);
            constexpr bool RK = decltype(rk)::value;
            hipLaunchKernelGGL(k_qb_gather<KeyQ>, grid_m, dim3(256), 0, st, static_cast<const KeyQ *>(qkeys), (const uint32_t *) w.recpos.as<uint32_t>(),
                               (const uint2 *) w.post.as<uint2>(), (const uint32_t *) pm_out, (const uint32_t *) qk_out, (const unsigned long long *) ctl, lay,
                               w.srank.as<KeyQ>(), w.spost.as<uint2>(), w.seg_off.as<uint32_t>());
            PDL_HIP(hipGetLastError());
            if constexpr (RK) pdl_query_rebase(c, w.srank.p, nullptr, ctl + Q_RUN_RECORDS, Mq);
            const QBView<KeyB, KeyQ, RK> v = qb_view<KeyB, KeyQ, RK>(c, qk_out);
            hipLaunchKernelGGL((k_qb_fold<KeyB, KeyQ, RK>), dim3((nq + 63) / 64), dim3(64), 0, st, v, nq, ctl, w.folds.as<QFold>());
            hipLaunchKernelGGL((k_qb_match<KeyB, KeyQ, RK>), grid_m, dim3(256), 0, st, v, (const QFold *) w.folds.as<QFold>(), lay, mo, Mq);
        });
        PDL_HIP(hipGetLastError());
        // (the records are segment positions now; every row's id in its own union comes with the offsets)
        rec_sorted = q_gene_rows(c, w, run, [&](const uint32_t *gene_sorted) {
            hipLaunchKernelGGL(k_qb_row_off, dim3((NT + 1 + 255) / 256), dim3(256), 0, st, gene_sorted, ctl, lay, N, w.row_off.as<uint32_t>(),
                               (const uint32_t *) w.row_lookups.as<uint32_t>(), QJ_LIMIT, w.rowid.as<uint32_t>());
        });
    }
    // the look, B-join, B-order: a row's arguments are those of its gene's query (qb_row_args); cells per query behind the order
    return q_join_and_order(c, w, run, w.spost.as<uint2>(), rec_sorted,
        [&](const QJoinArgs &a) { hipLaunchKernelGGL(k_qb_join, dim3(NT), dim3(QJ_T), 0, st, QBJoinArgs{a, lay, hbm_cols}); },
        [&](const QJoinArgs &a, uint32_t W) { hipLaunchKernelGGL(k_qb_join_hbm, dim3(W), dim3(QJ_T), 0, st, QBJoinArgs{a, lay, hbm_cols}); },
        [&] { hipLaunchKernelGGL(k_qb_counts, dim3((nq + 63) / 64), dim3(64), 0, st, (const uint32_t *) w.fin_off.as<uint32_t>(), lay, ctl); });
}

// B-copy: the chunk's cells and maxima come over in one piece each (7 copies per chunk, not per query) into pinned host
// memory — a DMA, no staging by the runtime — then every query's block is cut out on the host.  Appends the blocks to
// out[qa..) / info (a failure leaves the freeing to the caller).
static void qb_copy_chunk(pdl_ctx *c, const std::vector<QBQuery> &qs, uint32_t qa, const pdl_query_cells &ch, pdl_scores *out, pdl_query_info *info,
                          float *device_ms) {
    hipStream_t st = c->stream;
    PinBuf &stage = c->qbb.stage;
    const uint32_t N = c->N, G1 = c->G + 1, nq = ch.nq;
    const uint64_t Z = ch.Z, cap = ch.cap;
    const size_t ms_floats = (size_t) ch.genes * G1, cm_floats = (size_t) nq * N + ch.genes;
    const size_t stage_words = (size_t) Z * 5 + ms_floats + cm_floats;
    stage.alloc(stage_words * 4);
    const uint32_t *h_cells = reinterpret_cast<const uint32_t *>(stage.p);
    const float *h_ms = reinterpret_cast<const float *>(stage.p) + (size_t) Z * 5, *h_cm = h_ms + ms_floats;
    if (Z)
        for (int i = 0; i < 5; i++) PDL_HIP(hipMemcpyAsync(stage.p + (size_t) i * Z * 4, ch.cells + (size_t) i * cap, Z * 4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipMemcpyAsync(const_cast<float *>(h_ms), ch.MS, ms_floats * 4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipMemcpyAsync(const_cast<float *>(h_cm), ch.CM, cm_floats * 4, hipMemcpyDeviceToHost, st));
    PDL_HIP(hipStreamSynchronize(st));
    const float ms_total = ch.device_ms();
    *device_ms += ms_total;
    uint64_t z0 = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const QBQuery &Q = qs[qa + q];
        const uint64_t Zq = ch.cells_of[q];
        const uint32_t n = Q.n, NC = N + n;
        if (z0 + Zq > Z) PDL_FAIL(PDL_ERR_DEVICE, "query batch: the queries' cells (%llu) pass the emitted total %llu", (unsigned long long) (z0 + Zq), (unsigned long long) Z);
        pdl_scores &r = out[qa + q];                             // (filled in place: a throw leaves what is allocated to the caller's pdl_free_scores)
        q_block_alloc(c, r, Zq, n);
        void *dst[5] = {r.scores, r.percs, r.tr_percs, r.row, r.column};
        for (int i = 0; i < 5; i++) if (Zq) memcpy(dst[i], h_cells + (size_t) i * Z + z0, Zq * 4);
        memcpy(r.max_genome_score, h_ms + (size_t) ch.gene_begin[q] * G1, (size_t) n * G1 * 4);
        memcpy(r.max_genome_score_col, h_cm + (size_t) q * N + ch.gene_begin[q], (size_t) NC * 4);
        q_block_ids(c, r);
        z0 += Zq;
        if (info) ch.info_of(q, Q.Rq, Q.Mq, ms_total / (float) nq, &info[qa + q]);
    }
}

// What the host knows of every query before the device is asked, behind the domain refusals of a batch; -> columns the HBM tables
// of the join's last tier are laid out for.  column_bytes: what the caller's own stages hold per column of a query's union on top
// (K-place for a batch: its copy of the base's labels and the group table)
uint32_t pdl_query_batch_plan(pdl_ctx *c, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries, std::vector<QBQuery> &qs,
                              uint64_t column_bytes) {
    const uint32_t N = c->N, G1 = c->G + 1, k = c->rp.k;
    if (c->R + (offsets[n] - offsets[0]) >= 0xfffffff0ull) PDL_FAIL(PDL_ERR_UNSUPPORTED, "more than 2^32 residues in the base and the batch need 64-bit stream positions");
    if (c->max_kseq >= (1ull << 20)) PDL_FAIL(PDL_ERR_UNSUPPORTED, "a base gene of %llu k-mers: queries need genes below 2^20 k-mers", (unsigned long long) c->max_kseq);
    // (option "query_rekey": a chunk may be ranked with 64-bit keys over a 32-bit base, and Q-rebase leaves a base key and a flag per record)
    const size_t kb = (c->key64 || c->opt_query_rekey) ? 8 : 4, rebased = c->opt_query_rekey ? (c->key64 ? 8 : 4) + 1 : 0;
    qs.assign(n_queries, QBQuery{});
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
        Q.bytes = Q.Rq + Q.Mq * (3 * kb + rebased + 2 * 4 + 4 + 8 + 4 * 8 + 8 + sizeof(QDesc)) + ((uint64_t) N + Q.n) * (4 + column_bytes) + (uint64_t) Q.n * (G1 * 4ull + 48);
        n_max = std::max(n_max, Q.n);
    }
    return N + n_max;
}
// the chunk that starts at query qa: consecutive queries within the byte budget (and the 31-bit record positions); one query always goes
uint32_t pdl_query_batch_chunk_end(const pdl_ctx *c, const std::vector<QBQuery> &qs, uint32_t qa) {
    const uint32_t n_queries = (uint32_t) qs.size();
    uint32_t qe = qa + 1;
    uint64_t bytes = qs[qa].bytes, m = qs[qa].Mq;
    while (qe < n_queries && bytes + qs[qe].bytes <= c->opt_query_batch_bytes && m + qs[qe].Mq < 0x7ffff000ull) { bytes += qs[qe].bytes; m += qs[qe].Mq; qe++; }
    return qe;
}

void pdl_run_query_batch(pdl_ctx *c, const uint8_t *residues, const uint64_t *offsets, const uint32_t *gene_begin, uint32_t n, uint32_t n_queries,
                         pdl_scores *out, pdl_query_info *info, pdl_query_batch_info *binfo) {
    std::vector<QBQuery> qs;
    const uint32_t hbm_cols = pdl_query_batch_plan(c, offsets, gene_begin, n, n_queries, qs, 0);
    float device_ms = 0.f;
    uint32_t chunks = 0;
    for (uint32_t qa = 0; qa < n_queries;) {
        const uint32_t qe = pdl_query_batch_chunk_end(c, qs, qa);
        const pdl_query_cells ch = pdl_run_query_chunk_device(c, residues, offsets, qs, qa, qe, hbm_cols);
        qb_copy_chunk(c, qs, qa, ch, out, info, &device_ms);
        chunks++;
        qa += ch.nq;                                              // (option "query_rekey" may have cut the chunk short of qe)
    }
    if (binfo) { binfo->queries = n_queries; binfo->chunks = chunks; binfo->device_ms = device_ms; }
}
